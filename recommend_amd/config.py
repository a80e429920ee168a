"""OneTrans configuration — mirrors the reference's ``practice/config.py``.

Reference: ``rank/scaling_up/oneTrans/practice/config.py:9-121``.  The attribute
names, defaults, ``to_dict``/``from_dict`` and the small/default/large presets are
kept so a reference ``config.json`` (written by ``train.py:289-291``) loads
unchanged.  Build-only knobs (marked ``# build``) select between the reference's
literal semantics and the fixes recorded in DESIGN.md §Semantics:

* ``dedicated_positions`` — ``'head'`` reproduces ``model.py:69,155`` (positions
  ``< num_ns_tokens`` get the dedicated weights, i.e. the first tokens, which are
  S-tokens because the tokenizer concatenates ``[S; NS]`` at ``model.py:235``);
  ``'tail'`` gives them to the last ``num_ns_tokens`` tokens (paper eq. 12).
* ``pyramid_fix`` — the reference computes pyramid query indices against the
  *original* length (``model.py:293-296,343,349``) which is out of range from
  layer 1 on; the fix indexes against the current length ``I_l`` and caps
  ``keep_l`` at ``I_l``.  With the fix off, an out-of-range schedule raises
  ``IndexError`` (TF's CPU behaviour for the same gather).
* ``pyramid_select`` — which queries a pyramid layer keeps.  ``'tail'`` is the
  reference's static tail slice (``model.py:296, 371``); ``'norm'`` (build
  extension) keeps the NS tokens plus the S tokens of largest RMS (top-K per
  sample, ``ot_pyramid_select``), which needs ``dedicated_positions='tail'`` so
  the dedicated (NS) rows stay at fixed places.  Both run the same wavefront
  top-K kernel; 'tail' passes no score, so the position tie-break picks the tail.
* ``sparse_features`` / ``seq_item_vocab`` — the Criteo-shape embedding-gather
  extension (north_star): NS features named here carry int64 ids looked up in a
  per-field table of width ``ns_embedding_dim``; sequence features carry int64
  item ids looked up in one ``[seq_item_vocab, seq_feature_dim]`` table.
"""

from __future__ import annotations

import copy
import math
from typing import Dict, List, Optional, Tuple


class OneTransConfig:
    """Same attribute surface as the reference ``OneTransConfig`` (config.py:9-69)."""

    def __init__(self):
        # model architecture (config.py:14-18)
        self.hidden_dim = 384
        self.num_layers = 8
        self.num_heads = 4
        self.ffn_dim = 1536
        # inputs (config.py:20-23)
        self.max_seq_len = 2048
        self.num_ns_tokens = 12
        self.sep_token_id = 0
        # mixed parameterisation (config.py:25-27)
        self.shared_s_params = True
        self.dedicated_ns_params = True
        # pyramid (config.py:29-31)
        self.pyramid_enabled = True
        self.pyramid_ratios = [0.5, 0.3, 0.2, 0.1, 0.05, 0.03, 0.02, 0.01]
        # training (config.py:33-37)
        self.batch_size = 2048
        self.learning_rate = 0.005
        self.num_epochs = 100
        self.warmup_steps = 10000
        # optimiser (config.py:39-48)
        self.optimizer_config = {
            'dense_optimizer': 'rmsprop',
            'sparse_optimizer': 'adagrad',
            'dense_lr': 0.005,
            'sparse_lr': 0.1,
            'beta1': 0.1,
            'beta2': 1.0,
            'momentum': 0.99999,
        }
        # regularisation (config.py:50-53)
        self.dropout_rate = 0.1
        self.weight_decay = 0.0
        self.gradient_clip_norm = 90.0
        # features (config.py:55-61)
        self.feature_config = {
            'user_features': ['user_id', 'age', 'gender', 'location'],
            'item_features': ['item_id', 'category', 'price', 'brand'],
            'context_features': ['time', 'device', 'platform'],
            'sequence_features': ['click_seq', 'cart_seq', 'purchase_seq'],
        }
        # tasks (config.py:63-64)
        self.tasks = ['ctr', 'cvr']
        # system flags (config.py:66-70)
        self.use_mixed_precision = True
        self.use_kv_cache = True
        self.use_flash_attention = True
        self.use_activation_recompute = True

        # ---- build knobs (not in the reference) ----
        self.dedicated_positions = 'head'    # build: 'head' (ref model.py:69) | 'tail' (paper eq.12)
        self.pyramid_fix = True              # build: index pyramid against the current length
        self.pyramid_select = 'tail'         # build: 'tail' (ref model.py:296) | 'norm' (top-K by token RMS)
        self.seq_feature_dim = 64            # build: width of one sequence event (data_loader.py:146,322)
        self.ns_embedding_dim = 16           # build: per-field NS embedding width (Criteo shape)
        self.sparse_features: Dict[str, int] = {}   # build: NS id features -> cardinality
        # build: multi-valued NS id features, pooled on the device into one NS column block each.
        # name -> {'cardinality': N, 'pooling': 'sum' | 'mean'} (its own N rows of emb.ns, width ns_embedding_dim)
        # or {'table': 'seq_item', 'pooling': ...} (rows of emb.seq_item, width seq_feature_dim); pooling
        # defaults to 'mean'.  The input is an integer [B, cap] array, id < 0 or >= the row count = empty slot
        self.bag_features: Dict[str, Dict] = {}
        self.seq_item_vocab = 0              # build: >0 => sequence features are item ids
        self.compute_dtype = 'fp32'          # build: arithmetic of the HIP path (reference is fp32)
        # build: the behaviour behind two reference flags the reference itself never reads
        # (use_activation_recompute config.py:69, warmup_steps config.py:36), opt-in so default numerics and
        # memory match the reference: recompute each block's forward in its backward (keep only the block
        # input), and a linear warm-up of the dense LR over warmup_steps
        self.recompute_blocks = False
        self.apply_warmup = False
        self.sparse_clip_norm = 120.0        # build: paper clip for sparse grads (complete_translation.md:190)
        self.adagrad_initial_accumulator = 0.1   # build: Keras Adagrad default
        self.adagrad_epsilon = 1e-7              # build: Keras Adagrad default
        self.rmsprop_rho = 0.9                   # build: Keras RMSprop default (train.py:66 reads rho default)
        self.rmsprop_epsilon = 1e-7              # build: Keras RMSprop default (train.py:68)
        # build: how the behaviour sequences become the S tokens.  'sep' (the reference, model.py:256-277): whole
        # sequences concatenated, a learnable [SEP] after each but the last.  'time' (the paper's default,
        # timestamp-aware): every event interleaved by its time, no [SEP]; each present sequence ``name`` then
        # needs integer times ``seq_features[name + seq_time_suffix]`` [B, L_name] (DESIGN.md §Sequence fusion)
        self.seq_fusion = 'sep'
        self.seq_time_suffix = '_time'
        # build: variable-length histories.  On: each present sequence ``name`` carries
        # ``seq_features[name + seq_len_suffix]``, an integer [B] count of real events (the last ``len`` positions, as
        # SequenceProcessor.pad_batch lays them out), and padding events are masked out as attention keys.  Off (the
        # reference): a padding event is an ordinary token and nothing new is read
        self.seq_padding_mask = False
        self.seq_len_suffix = '_len'
        # build: how the NS features become the L_NS non-sequence tokens (paper §3.2.1).  'auto' (the
        # reference, eq. 7): one Dense(F_ns -> L_NS*d) cut into tokens.  'group' (eq. 6): ``ns_token_groups``, a list
        # of num_ns_tokens lists of NS feature names that partition ns_feature_names(), and group g goes through its
        # own Dense(F_g -> d) to become token g
        self.ns_tokenizer = 'auto'
        self.ns_token_groups: List[List[str]] = []
        # build: weighted and partially labelled multi-task training.  Off (the reference): every
        # sample counts once in every task and nothing new is read.  On: the labels dict may carry
        # ``labels[sample_weight_key]`` and ``labels[task + label_weight_suffix]`` ([B] or [B, 1], in [0, 65536]); task
        # t weighs sample b by their product (a missing factor is 1, a zero removes the entry, whose label may then be
        # NaN), in the loss, its gradient and the running metrics.  ``task_loss_weights`` {task: a_t} scales a task's
        # loss term (never a metric; a missing task is 1).  ``loss_reduction``: 'batch' divides a task's weighted sum
        # by B (Keras SUM_OVER_BATCH_SIZE with sample_weight), 'weights' by the task's sum of weights
        self.weighted_loss = False
        self.loss_reduction = 'batch'
        self.task_loss_weights: Dict[str, float] = {}
        self.sample_weight_key = 'sample_weight'
        self.label_weight_suffix = '_weight'

    # ------------------------------------------------------------------ helpers
    def to_dict(self) -> Dict:
        """config.py:71-73."""
        return {k: copy.deepcopy(v) for k, v in self.__dict__.items() if not k.startswith('_')}

    @classmethod
    def from_dict(cls, config_dict: Dict) -> 'OneTransConfig':
        """config.py:75-82: unknown keys are ignored, known keys overwrite."""
        config = cls()
        for key, value in config_dict.items():
            if hasattr(config, key):
                setattr(config, key, copy.deepcopy(value))
        return config

    # derived quantities -------------------------------------------------------
    @property
    def head_dim(self) -> int:
        return self.hidden_dim // self.num_heads

    @property
    def num_groups(self) -> int:
        """Weight groups of the mixed parameterisation: 0 = shared, 1..L_NS = dedicated."""
        return 1 + self.num_ns_tokens

    def ns_feature_names(self) -> List[str]:
        """Concat order of NS features (model.py:243-247)."""
        fc = self.feature_config
        return list(fc['user_features']) + list(fc['item_features']) + list(fc['context_features'])

    def ns_feature_width(self, name: str) -> int:
        """Columns of one NS feature in the concat: 1 (dense), ns_embedding_dim (sparse id, or a bag over its own
        rows of emb.ns), seq_feature_dim (a bag over emb.seq_item)."""
        bag = getattr(self, 'bag_features', {}).get(name)
        if bag is not None:
            return self.seq_feature_dim if bag.get('table') == 'seq_item' else self.ns_embedding_dim
        return self.ns_embedding_dim if name in self.sparse_features else 1

    def bag_pooling(self, name: str) -> str:
        return self.bag_features[name].get('pooling', 'mean')

    def bag_rows(self, name: str) -> int:
        """Row count a bag's ids are checked against: its cardinality, or seq_item_vocab."""
        bag = self.bag_features[name]
        return int(self.seq_item_vocab if bag.get('table') == 'seq_item' else bag['cardinality'])

    def ns_input_width(self, present: Optional[List[str]] = None) -> int:
        """F_ns: 1 per dense feature, ns_embedding_dim per sparse-id feature, the table width per bag feature."""
        names = self.ns_feature_names() if present is None else present
        return sum(self.ns_feature_width(n) for n in names)

    def seq_token_count(self, seq_lens: List[int]) -> int:
        """L_S = sum(L_i) + one [SEP] after every present sequence i < n-1 (model.py:266-272); no [SEP] under
        ``seq_fusion='time'``."""
        n = len(self.feature_config['sequence_features'])
        if len(seq_lens) != n:
            return None
        return int(sum(seq_lens)) + (max(0, n - 1) if getattr(self, 'seq_fusion', 'sep') == 'sep' else 0)

    def pyramid_schedule(self, total_seq_len: int) -> List[Dict]:
        """Per layer (in_len I_l, keep K_l).  Follows PyramidScheduler.get_layer_config
        (model.py:287-302) with the D2 fix: keep_l = max(1, int(L0*ratio_l)) capped at I_l and
        the kept queries are the tail of the *current* sequence.  The last layer keeps
        exactly 1 token downstream (only output_tokens[:, -1] is read at model.py:390),
        which is recorded as ``needed`` (dead-code elimination, exact)."""
        sched = []
        cur = total_seq_len
        for l in range(self.num_layers):
            if self.pyramid_enabled and l < len(self.pyramid_ratios):
                keep = max(1, int(total_seq_len * self.pyramid_ratios[l]))
                if self.pyramid_fix:
                    keep = min(keep, cur)
                elif total_seq_len > cur:
                    # reference gathers range(L0-keep, L0) from a tensor of length cur < L0
                    raise IndexError('pyramid gather out of range (reference defect D2)')
            else:
                keep = cur
            sched.append({'in_len': cur, 'keep': keep})
            cur = keep
        # the model reads only the last token of the final layer
        for l, s in enumerate(sched):
            s['needed'] = s['keep'] if l < len(sched) - 1 else 1
        return sched

    def group_of_position(self, p: int, in_len: int) -> int:
        """Weight group for position p of a layer whose input has in_len tokens.
        'head': model.py:69 (`idx < num_ns_tokens` -> dedicated[idx]); 'tail': paper eq. 12."""
        if self.dedicated_positions == 'head':
            return 1 + p if p < self.num_ns_tokens else 0
        if self.dedicated_positions == 'tail':
            j = p - (in_len - self.num_ns_tokens)
            return 1 + j if j >= 0 else 0
        raise ValueError(f'unknown dedicated_positions {self.dedicated_positions!r}')


class OneTransSmallConfig(OneTransConfig):
    """config.py:85-92."""

    def __init__(self):
        super().__init__()
        self.hidden_dim = 256
        self.num_layers = 6
        self.ffn_dim = 1024


class OneTransLargeConfig(OneTransConfig):
    """config.py:95-103."""

    def __init__(self):
        super().__init__()
        self.hidden_dim = 512
        self.num_layers = 12
        self.num_heads = 8
        self.ffn_dim = 2048


def get_model_config(model_type: str = 'default') -> OneTransConfig:
    """config.py:106-117: ValueError on an unknown preset (same as the reference)."""
    config_map = {
        'small': OneTransSmallConfig,
        'default': OneTransConfig,
        'large': OneTransLargeConfig,
    }
    if model_type not in config_map:
        raise ValueError(f"unknown model type: {model_type}")
    return config_map[model_type]()


def dense_optimizer_spec(config: OneTransConfig) -> Tuple[str, Dict[str, float]]:
    """The dense optimizer ``optimizer_config['dense_optimizer']`` selects, as the reference's
    ``_create_optimizer`` does (train.py:53-76): ``(kind, params)``.

    * ``'rmsprop'``: Keras RMSprop — ``{lr, rho, eps, momentum}`` (rho / eps: ``rmsprop_rho`` /
      ``rmsprop_epsilon``; momentum: ``optimizer_config['momentum']``, 0 without it).
    * ``'adam'``: Keras Adam — ``{lr, beta1, beta2, eps}`` from ``optimizer_config['beta1' / 'beta2' /
      'epsilon']``, 0.9 / 0.999 / 1e-8 without them (train.py:60-62).
    * any other name, or none: the reference falls back to ``tf.keras.optimizers.Adam`` with only the
      learning rate given (train.py:71-74), i.e. the Keras defaults beta1 0.9, beta2 0.999, epsilon 1e-7;
      ``beta1`` / ``beta2`` / ``epsilon`` of ``optimizer_config`` are not read on this branch.

    ``lr`` is ``optimizer_config['dense_lr']``, else ``config.learning_rate``.  (The reference reads
    ``optimizer_config['learning_rate']``, a key its own default dict does not have, so it raises KeyError on its
    own defaults; that key is not read here.)"""
    oc = config.optimizer_config
    lr = float(oc.get('dense_lr', config.learning_rate))
    name = oc.get('dense_optimizer')
    if name == 'rmsprop':
        return 'rmsprop', {'lr': lr, 'rho': float(config.rmsprop_rho), 'eps': float(config.rmsprop_epsilon),
                           'momentum': float(oc.get('momentum', 0.0))}
    if name == 'adam':
        return 'adam', {'lr': lr, 'beta1': float(oc.get('beta1', 0.9)), 'beta2': float(oc.get('beta2', 0.999)),
                        'eps': float(oc.get('epsilon', 1e-8))}
    return 'adam', {'lr': lr, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-7}


SPARSE_OPTIMIZERS = ('adagrad', 'rowwise_adagrad')


def sparse_optimizer_spec(config: OneTransConfig) -> Tuple[str, Dict[str, float]]:
    """The embedding-table optimizer ``optimizer_config['sparse_optimizer']`` selects: ``(kind, params)`` with
    params ``{lr, eps, initial_accumulator, clip}`` (``optimizer_config['sparse_lr']``, ``adagrad_epsilon``,
    ``adagrad_initial_accumulator``, ``sparse_clip_norm``).

    * ``'adagrad'`` (the default, also without the key): element-wise Keras Adagrad, one accumulator per element.
    * ``'rowwise_adagrad'``: one accumulator per table row, ``A[r] += mean_c g[r, c]^2``.
    * any other name: ValueError.  (Unlike the dense side, where the reference itself falls back to Adam, the
      reference never reads this key: there is no fallback to mirror, and a name that is silently ignored is a bug.)"""
    oc = config.optimizer_config
    name = oc.get('sparse_optimizer', 'adagrad')
    if name not in SPARSE_OPTIMIZERS:
        raise ValueError(f'unknown sparse_optimizer {name!r}: expected one of {list(SPARSE_OPTIMIZERS)}')
    return name, {'lr': float(oc.get('sparse_lr', 0.1)), 'eps': float(config.adagrad_epsilon),
                  'initial_accumulator': float(config.adagrad_initial_accumulator),
                  'clip': float(config.sparse_clip_norm)}


DEFAULT_CONFIG = OneTransConfig()

# ---------------------------------------------------------------------------
# BASELINE.json workloads.  B and L_NS values not fixed by
# BASELINE.json are builder choices, reported in DESIGN.md.
# ---------------------------------------------------------------------------

# 26 Criteo-like categorical fields, cardinalities log-spaced 1e3 .. 1e7
CRITEO_CARDINALITIES = [int(round(10 ** (3 + 4 * i / 25))) for i in range(26)]


def _criteo_features(cfg: OneTransConfig, seq_lens: List[int], item_vocab: int) -> None:
    dense = [f'I{i}' for i in range(1, 14)]
    sparse = [f'C{i}' for i in range(1, 27)]
    cfg.feature_config = {
        'user_features': sparse[:13],
        'item_features': sparse[13:],
        'context_features': dense,
        'sequence_features': ['click_seq', 'cart_seq', 'purchase_seq'],
    }
    cfg.sparse_features = {name: card for name, card in zip(sparse, CRITEO_CARDINALITIES)}
    cfg.seq_item_vocab = item_vocab
    cfg._seq_lens = list(seq_lens)


def check_pyramid_select(cfg: OneTransConfig) -> None:
    """``pyramid_select`` is 'tail' (reference) or 'norm' (needs the NS tokens at the dedicated tail)."""
    sel = getattr(cfg, 'pyramid_select', 'tail')
    if sel not in ('tail', 'norm'):
        raise ValueError(f'unknown pyramid_select {sel!r}')
    if sel == 'norm' and cfg.dedicated_positions != 'tail':
        raise ValueError("pyramid_select='norm' needs dedicated_positions='tail' (the kept NS rows keep their "
                         "dedicated weights)")


def check_seq_fusion(cfg: OneTransConfig) -> None:
    """``seq_fusion`` is 'sep' (reference: concatenation with [SEP]) or 'time' (timestamp-aware interleave)."""
    mode = getattr(cfg, 'seq_fusion', 'sep')
    if mode not in ('sep', 'time'):
        raise ValueError(f"unknown seq_fusion {mode!r}: expected 'sep' or 'time'")
    if mode == 'time' and not getattr(cfg, 'seq_time_suffix', '_time'):
        raise ValueError("seq_fusion='time' needs a non-empty seq_time_suffix")


LOSS_REDUCTIONS = ('batch', 'weights')
LOSS_WEIGHT_MAX = 65536.0            # a sample / task weight lives in [0, 2^16] (ot_task_loss_weighted_*)


def check_weighted_loss(cfg: OneTransConfig) -> None:
    """``loss_reduction`` is 'batch' or 'weights'; every ``task_loss_weights`` key names a task and its value is a
    finite number >= 0; the two weight-key names are non-empty and distinct from the task names.  Nothing is checked
    while ``weighted_loss`` is off (none of these fields is then read)."""
    if not getattr(cfg, 'weighted_loss', False):
        return
    red = getattr(cfg, 'loss_reduction', 'batch')
    if red not in LOSS_REDUCTIONS:
        raise ValueError(f"unknown loss_reduction {red!r}: expected 'batch' or 'weights'")
    for t, a in (getattr(cfg, 'task_loss_weights', None) or {}).items():
        if t not in cfg.tasks:
            raise ValueError(f'task_loss_weights names {t!r}, which is not a task (tasks: {list(cfg.tasks)})')
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or a < 0:
            raise ValueError(f'task_loss_weights[{t!r}] = {a!r}: a finite number >= 0 expected')
    key, suf = getattr(cfg, 'sample_weight_key', 'sample_weight'), getattr(cfg, 'label_weight_suffix', '_weight')
    if not key or not suf:
        raise ValueError('weighted_loss needs a non-empty sample_weight_key and label_weight_suffix')
    if key in cfg.tasks or any(t + suf in cfg.tasks for t in cfg.tasks):
        raise ValueError('sample_weight_key / label_weight_suffix collide with a task name')


def task_loss_scale(cfg: OneTransConfig):
    """[a_t for t in tasks] from ``task_loss_weights``, or None when every coefficient is 1."""
    tw = getattr(cfg, 'task_loss_weights', None) or {}
    a = [float(tw.get(t, 1.0)) for t in cfg.tasks]
    return None if all(v == 1.0 for v in a) else a


def check_padding_mask(cfg: OneTransConfig) -> None:
    """``seq_padding_mask`` runs the masked f32-accurate attention kernels over tail keeps only: the reduced-precision
    attention kernels carry no mask, and a score-based pyramid keep would have to exclude padding tokens."""
    if not getattr(cfg, 'seq_padding_mask', False):
        return
    if not getattr(cfg, 'seq_len_suffix', '_len'):
        raise ValueError('seq_padding_mask needs a non-empty seq_len_suffix')
    if getattr(cfg, 'compute_dtype', 'fp32') in ('bf16', 'fp8attn'):
        raise NotImplementedError(f"seq_padding_mask with compute_dtype {cfg.compute_dtype!r}: the bf16 and fp8 "
                                  "attention kernels carry no padding mask; use compute_dtype 'fp32'")
    if getattr(cfg, 'pyramid_select', 'tail') == 'norm':
        raise ValueError("seq_padding_mask with pyramid_select='norm': a score-based keep would have to exclude "
                         "padding tokens (not implemented); use pyramid_select='tail'")


def check_ns_tokenizer(cfg: OneTransConfig) -> None:
    """``ns_tokenizer`` is 'auto' (reference: one Dense cut into tokens) or 'group' (one Dense per feature group);
    'group' needs ``ns_token_groups``: num_ns_tokens non-empty lists of NS feature names, every name of
    ``ns_feature_names()`` in exactly one of them."""
    mode = getattr(cfg, 'ns_tokenizer', 'auto')
    if mode not in ('auto', 'group'):
        raise ValueError(f"unknown ns_tokenizer {mode!r}: expected 'auto' or 'group'")
    if mode == 'auto':
        return
    groups = getattr(cfg, 'ns_token_groups', None)
    if not groups:
        raise ValueError("ns_tokenizer='group' needs ns_token_groups (num_ns_tokens lists of NS feature names)")
    if len(groups) != cfg.num_ns_tokens:
        raise ValueError(f'ns_token_groups has {len(groups)} groups, num_ns_tokens is {cfg.num_ns_tokens}')
    names = cfg.ns_feature_names()
    seen = {}
    for g, members in enumerate(groups):
        if isinstance(members, str) or not len(members):
            raise ValueError(f'ns_token_groups[{g}] is empty (or not a list of names)')
        for n in members:
            if n not in names:
                raise ValueError(f'ns_token_groups[{g}]: {n!r} is in none of the user / item / context feature lists')
            if n in seen:
                raise ValueError(f'ns_token_groups: feature {n!r} is in groups {seen[n]} and {g}')
            seen[n] = g
    missing = [n for n in names if n not in seen]
    if missing:
        raise ValueError(f'ns_token_groups: features {missing} are in no group')


def ns_group_mode(cfg: OneTransConfig) -> bool:
    return getattr(cfg, 'ns_tokenizer', 'auto') == 'group'


def ns_group_layout(cfg: OneTransConfig) -> Dict:
    """Rows of the group-major ``tok.ns.kernel`` [F_ns, d], which are also the columns of the NS matrix, under
    ns_tokenizer='group'.  Inside a group the features follow concat order (``ns_feature_names()``),
    ``ns_feature_width`` rows each; the groups are not padded (the kernels assume no alignment of a group's range).

    * ``members``: the groups' features in that order; ``widths``: F_g per group.
    * ``goff`` [G+1]: the groups' first rows, goff[G] = F_ns; ``col``: feature -> its first row / column."""
    check_ns_tokenizer(cfg)
    order = {n: i for i, n in enumerate(cfg.ns_feature_names())}
    members = [sorted(g, key=order.__getitem__) for g in cfg.ns_token_groups]
    goff, col, widths = [0], {}, []
    for g in members:
        r = goff[-1]
        for n in g:
            col[n] = r
            r += cfg.ns_feature_width(n)
        widths.append(r - goff[-1])
        goff.append(r)
    return {'members': members, 'widths': widths, 'goff': goff, 'col': col}


def even_ns_groups(cfg: OneTransConfig) -> List[List[str]]:
    """``ns_feature_names()`` cut, in concat order, into num_ns_tokens contiguous runs of near-equal column width: run
    g ends at the feature whose end column is nearest to (g+1)/L of the total, every run keeping at least one
    feature.  Needs at least num_ns_tokens features."""
    names = cfg.ns_feature_names()
    L = cfg.num_ns_tokens
    if len(names) < L:
        raise ValueError(f'even_ns_groups: {len(names)} NS features cannot fill {L} groups')
    ends = []
    c = 0
    for n in names:
        c += cfg.ns_feature_width(n)
        ends.append(c)
    total, groups, start = c, [], 0
    for g in range(L):
        if g == L - 1:
            stop = len(names)
        else:
            lo, hi = start + 1, len(names) - (L - 1 - g)          # leave a feature for every later run
            target = total * (g + 1) / L
            stop = min(range(lo, hi + 1), key=lambda i: (abs(ends[i - 1] - target), i))
        groups.append(names[start:stop])
        start = stop
    return groups


BAG_POOLINGS = ('sum', 'mean')


def check_bag_features(cfg: OneTransConfig) -> None:
    """``bag_features``: every name is an NS feature that is not also in ``sparse_features``; each entry names
    either a cardinality (own rows of emb.ns) or ``table='seq_item'`` (needs ``seq_item_vocab > 0``), and a
    pooling of 'sum' or 'mean'."""
    bags = getattr(cfg, 'bag_features', None) or {}
    names = cfg.ns_feature_names()
    for name, spec in bags.items():
        if name in cfg.sparse_features:
            raise ValueError(f'bag feature {name!r} is also in sparse_features')
        if name not in names:
            raise ValueError(f'bag feature {name!r} is in none of the user / item / context feature lists')
        if not isinstance(spec, dict):
            raise ValueError(f'bag feature {name!r}: a dict is expected, got {spec!r}')
        pooling = spec.get('pooling', 'mean')
        if pooling not in BAG_POOLINGS:
            raise ValueError(f"bag feature {name!r}: unknown pooling {pooling!r}: expected 'sum' or 'mean'")
        if 'table' in spec:
            if spec['table'] != 'seq_item':
                raise ValueError(f"bag feature {name!r}: unknown table {spec['table']!r}: expected 'seq_item'")
            if 'cardinality' in spec:
                raise ValueError(f"bag feature {name!r}: give either 'cardinality' or 'table', not both")
            if not cfg.seq_item_vocab:
                raise ValueError(f"bag feature {name!r}: table 'seq_item' needs seq_item_vocab > 0")
        elif int(spec.get('cardinality', 0)) <= 0:
            raise ValueError(f"bag feature {name!r}: needs a positive 'cardinality' or table='seq_item'")


def workload_config(name: str) -> OneTransConfig:
    """Configs of BASELINE.json as OneTransConfig objects; ``cfg._seq_lens`` and
    ``cfg._batch`` carry the synthetic input shape."""
    cfg = OneTransConfig()
    cfg.pyramid_enabled = False
    name = name.upper()
    if name == 'C1':     # 2L d64, 8 NS + 32 S tokens, B512, reference-literal features
        cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.ffn_dim = 64, 2, 4, 256
        cfg.num_ns_tokens = 8
        cfg._seq_lens = [10, 10, 10]
        cfg._batch = 512
    elif name in ('C2', 'T'):   # 4L d128 (T: d256), L_NS 12, L_S 128 = 42*3+2, B4096
        d = 128 if name == 'C2' else 256
        cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.ffn_dim = d, 4, 4, 4 * d
        cfg.num_ns_tokens = 12
        _criteo_features(cfg, [42, 42, 42], 1_000_000)
        cfg._batch = 4096
    elif name == 'C3':   # 6L d256, L_S 512 = 170*3+2, pyramid 0.5/layer, B2048
        cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.ffn_dim = 256, 6, 4, 1024
        cfg.num_ns_tokens = 12
        cfg.pyramid_enabled = True
        cfg.pyramid_ratios = [0.5 ** (l + 1) for l in range(6)]
        _criteo_features(cfg, [170, 170, 170], 1_000_000)
        cfg._batch = 2048
    elif name == 'C4':   # 8L d256, L0 140, B2048/GPU, 100M-row item table row-sharded
        cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.ffn_dim = 256, 8, 4, 1024
        cfg.num_ns_tokens = 12
        _criteo_features(cfg, [42, 42, 42], 100_000_000)
        cfg._batch = 2048
    elif name == 'C5':   # 12L d512 H8, L_S 1024 = 341+341+340+2, B512/GPU
        cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.ffn_dim = 512, 12, 8, 2048
        cfg.num_ns_tokens = 12
        _criteo_features(cfg, [341, 341, 340], 1_000_000)
        cfg._batch = 512
    else:
        raise ValueError(f'unknown workload {name!r}')
    return cfg


def algorithmic_flops_per_sample(cfg: OneTransConfig, seq_lens: List[int], f_ns: int) -> Dict[str, float]:
    """SURVEY §8d exact minimal work (fwd), counting tail-only queries and the
    single needed query of the final layer.  fwd+bwd = 3 x fwd."""
    d, f = cfg.hidden_dim, cfg.ffn_dim
    L_S = cfg.seq_token_count(seq_lens)
    L0 = L_S + cfg.num_ns_tokens
    sched = cfg.pyramid_schedule(L0)
    attn = layers = 0.0
    for s in sched:
        I, K = s['in_len'], s['needed']
        P = K * I - K * (K - 1) / 2.0
        a = 4.0 * P * d
        attn += a
        layers += 4.0 * I * d * d + 2.0 * K * d * d + a + 2.0 * K * d * d + 4.0 * K * d * f
    tok = 2.0 * sum(seq_lens) * cfg.seq_feature_dim * d + 2.0 * f_ns * cfg.num_ns_tokens * d
    heads = len(cfg.tasks) * (2.0 * d * (d // 2) + 2.0 * (d // 2))
    fwd = layers + tok + heads
    return {'fwd': fwd, 'fwd_bwd': 3.0 * fwd, 'attn_fwd': attn}


__all__ = ['OneTransConfig', 'OneTransSmallConfig', 'OneTransLargeConfig', 'get_model_config',
           'dense_optimizer_spec', 'sparse_optimizer_spec', 'SPARSE_OPTIMIZERS', 'DEFAULT_CONFIG', 'workload_config', 'algorithmic_flops_per_sample',
           'CRITEO_CARDINALITIES', 'check_bag_features', 'check_ns_tokenizer', 'even_ns_groups', 'ns_group_layout',
           'ns_group_mode']
