"""Two-stage cached serving of a trained OneTrans model (paper §3.5.1 "cross-request KV cache").

Reference: the inference engine ``examples/inference_example.py:21-219`` (one full forward per batch
of (user, item, context, sequence) samples) and the model's KV-cache path ``model.py:94-98, 333,
359-381, 395-397``, which is defective (D6: block i's K/V are fed to block i+1 and the causal mask is
not offset by the cache length), so the cache semantics are re-derived from the paper:

* stage I, once per request (user): the S tokens (sequences + [SEP]) run through every layer on their
  own.  Tokens are ordered [S; NS] (model.py:235) and the mask is causal, so no S token ever sees an
  NS token: the S-side hidden states, keys and values do not depend on the candidate.  Each layer's
  S-side K/V rows are cached (``RequestCache``).
* stage II, once per candidate: the NS tokens run through every layer; their queries attend to the
  request's cached S-side K/V plus their own (``ot_attn_fwd_cached``).  Nothing S-side is recomputed.

The result equals ``OneTransModel.forward`` on the expanded batch (each candidate paired with its
request's sequences) up to fp32 summation order — tests/test_serving_gpu.py checks it against the
model and the CPU oracle.  Pyramid keeps (tail, model.py:296/371 with the D2 fix) and the last-layer
dead-code elimination carry over: at layer l the kept tail of K_l tokens splits into S rows (computed
in stage I) and N rows (stage II).  Inference only (no dropout).  Positions restart in every layer,
so every row's weight group is the one of its position in the full layer input
(``OneTransModel.maps(p0=, I_full=)``).

Cross-request reuse (``extend_requests``): new behaviours appended to the LAST configured sequence
extend the S side at its end, so with no pruning before the last layer only the new tokens are computed
(their queries over the cached K/V).  Appends anywhere else shift later positions (later sequences,
[SEP] tokens, position-grouped weights) and need a full stage-I re-encode; that case raises.
Under ``seq_fusion='time'`` the S side is ordered by event time and has no [SEP]: new events of any present
sequence land at its end as long as they are later than the request's cached latest event
(``RequestCache.last_time``), so every behaviour can extend the cache.

Cache precision (``OneTransServer(model, cache_dtype='bf16')``): the cached K/V rows stored rounded to
bf16, one buffer per layer that ``extend_requests`` grows in place; the default 'fp32' keeps the f32 qkv rows.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import kernels as K
from ._lib import OneTransHipError
from .span_block import check_req, request_schedule, s_rows, span_forward


def _cache_valid(valid, L_S: int, s: int):
    """The key-padding mask of a layer's s S rows — the last s of the L_S columns of ``valid`` [R, L_S] (tail keep) — as
    the kernels take it (tensor, element offset, row stride), or None without a mask."""
    return None if valid is None else (valid, L_S - s, L_S)


CACHE_DTYPES = ('fp32', 'bf16')


def bf16_cache_nbytes(cfg, R: int, L_S: int, reserve: int = 0) -> int:
    """Bytes of the K/V storage of a bf16 request cache: R · Σ_l cap_l · 2d · 2 with cap_l = Ic_l + reserve rows per
    request in layer l (Ic_l: the layer's S rows, ``request_schedule``).  The fp32 cache keeps Ic_l · 3d · 4 a row."""
    return R * sum(e['s'] + reserve for e in request_schedule(cfg, L_S)) * 2 * cfg.hidden_dim * 2


class RequestCache:
    """Stage-I output for R requests, per layer Ic (the number of S tokens in that layer's input) and their K/V:
    ``dtype`` 'fp32': 'kv', the S-side qkv rows [R*Ic, 3d] (k at col d, v at 2d);
    ``dtype`` 'bf16': 'kv16', one bfloat16 buffer [R, cap, 2d] (k at col 0, v at col d) whose first Ic rows of every
    request are this cache's; 'cap' its rows per request and 'high' a one-element list, shared by the caches that
    share the buffer, of the rows filled in it (``extend_requests`` appends in place behind them)."""

    def __init__(self, R: int, L_S: int, layers: List[Dict], present=(), last_time: Optional[torch.Tensor] = None,
                 valid: Optional[torch.Tensor] = None, dtype: str = 'fp32'):
        self.R, self.L_S, self.layers = R, L_S, layers
        self.dtype = dtype
        # seq_padding_mask: the S tokens' validity, uint8 [R, L_S]; a layer with Ic cached rows reads its last Ic columns
        self.valid = valid
        self.present = tuple(present)          # sequence names present in the requests, config order
        # seq_fusion='time': each request's latest event time, [R] int64 on the device (ot_seq_time_rows);
        # extend_requests appends only events after it
        self.last_time = last_time

    def nbytes(self) -> int:
        """Bytes of the K/V storage this cache holds (a bf16 buffer counts whole, reserve rows included)."""
        ts = [lay.get('kv16' if self.dtype == 'bf16' else 'kv') for lay in self.layers]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)


class OneTransServer:
    """Cached two-stage inference on a ``OneTransModel`` (weights shared, nothing copied).

    ``cache_dtype`` 'bf16': the request cache keeps each layer's S-side K/V rounded to bf16 (round to nearest even),
    a third of the fp32 cache's bytes (which also holds the Q columns).  Rounding happens only when a row is
    stored: stage I's own self-attention runs on the un-rounded f32 rows, a candidate's own rows stay f32, and the
    cached attention (ot_attn_fwd_cached_kv16) is exact in f32 over [rounded cache ; own rows] — the scores equal the
    fp32 server's on a cache whose K/V columns were rounded, up to f32 summation order."""

    def __init__(self, model, cache_dtype: str = 'fp32'):
        if cache_dtype not in CACHE_DTYPES:
            raise ValueError(f'OneTransServer: cache_dtype {cache_dtype!r}, expected one of {CACHE_DTYPES}')
        self.cache_dtype = cache_dtype
        self.m = model
        cfg = model.config
        if getattr(cfg, 'pyramid_select', 'tail') != 'tail':
            raise ValueError("OneTransServer: pyramid_select must be 'tail' (a score-based keep would depend on "
                             "the NS tokens' positions in every layer)")

    # ------------------------------------------------------------------ schedule

    @property
    def precision_model(self):
        """The model whose arithmetic the cached stages run in (kernels.in_model_precision)."""
        return self.m

    def schedule(self, L_S: int) -> List[Dict]:
        """Per layer: S rows s, N rows n, kept S rows kS, kept N rows kN (kS + kN = the layer's keep)."""
        return request_schedule(self.m.config, L_S)

    # ------------------------------------------------------------------ stage I
    @torch.no_grad()
    @K.in_model_precision
    def encode_requests(self, seq_features: Dict[str, torch.Tensor], reserve: int = 0) -> RequestCache:
        """Tokenize the requests' sequences (model.py:256-277) and run the S side of every layer;
        cache each layer's S-side K/V.  ``reserve`` (cache_dtype 'bf16'): rows per request every layer's buffer
        holds beyond its Ic, for ``extend_requests`` to append in place."""
        from .model import _Tokenize
        m = self.m
        cfg = m.config
        reserve = int(reserve)
        if reserve < 0:
            raise ValueError(f'encode_requests: reserve={reserve} is negative')
        if not seq_features:
            raise ValueError('encode_requests: no sequence features')
        plan = m._plan({}, seq_features)
        R, L_S = plan['B'], plan['L_S']
        x = s_rows(_Tokenize.apply(m.flat, m, plan), plan)                # NS rows zero (no NS features)
        # seq_padding_mask: the S columns of the plan's validity array (its lengths come with seq_features)
        valid = plan['valid0'][:, :L_S].contiguous() if m.padding_mask else None
        bf16 = self.cache_dtype == 'bf16'
        layers = []
        for l, e in enumerate(self.schedule(L_S)):
            s, kS = e['s'], e['kS']
            if s == 0:
                layers.append(self._kv16_layer(None, R, 0, reserve, 0) if bf16 else {'Ic': 0, 'kv': None})
                continue
            x, qkv, _ = span_forward(m, l, x, R, s, kS, 0, e['I'], cached=False,     # S queries see S keys only
                                     valid=_cache_valid(valid, L_S, s))
            # bf16: the rounded K | V rows are all that stays (qkv, with its Q columns, is dropped here)
            layers.append(self._kv16_layer(qkv, R, s, s + reserve, 0) if bf16 else {'Ic': s, 'kv': qkv})
        present = [n for n in cfg.feature_config['sequence_features'] if n in seq_features]
        last_time = plan['last_time'].clone() if m.time_fusion else None
        return RequestCache(R, L_S, layers, present, last_time, valid, self.cache_dtype)

    def _kv16_layer(self, qkv, R: int, rows: int, cap: int, Ic: int, old: Optional[Dict] = None) -> Dict:
        """A bf16 cache layer of ``Ic + rows`` rows: the K | V columns of ``qkv`` [R*rows, 3d] packed behind the Ic
        rows of layer ``old`` — in its buffer when they fit and the buffer ends at those Ic rows (its high-water
        mark), else in a new buffer of ``cap`` rows per request that takes one copy of them."""
        d = self.m.config.hidden_dim
        if old is not None and Ic + rows <= old['cap'] and old['high'][0] == Ic:
            buf, cap, high = old['kv16'], old['cap'], old['high']
        else:
            buf, high = torch.empty(R, cap, 2 * d, dtype=torch.bfloat16, device=self.m.device), [Ic]
            if Ic > 0:
                buf[:, :Ic] = old['kv16'][:, :Ic]
        if rows > 0:
            K.kv_pack_bf16(qkv, 3 * d, R, rows, d, buf, 2 * d, cap, Ic)
        high[0] = Ic + rows
        return {'Ic': Ic + rows, 'kv16': buf, 'cap': cap, 'high': high}

    def _check_cache(self, who: str, cache: RequestCache) -> None:
        if cache.dtype != self.cache_dtype:
            raise ValueError(f'{who}: a {cache.dtype!r} request cache was given to a server with cache_dtype '
                             f'{self.cache_dtype!r}')

    # ------------------------------------------------------------------ cross-request append
    @torch.no_grad()
    @K.in_model_precision
    def extend_requests(self, cache: RequestCache, seq_name: str, new_events: torch.Tensor,
                        new_times: Optional[torch.Tensor] = None) -> RequestCache:
        """Cross-request KV cache (paper §3.5.1): the requests' newest behaviours ``new_events``
        ([R, dL, 64] features or [R, dL] ids) are appended to sequence ``seq_name`` and only the new
        S tokens are computed, their queries attending over the cached K/V (ot_attn_fwd_cached).

        Exact (equal to encode_requests on the extended sequences) when the appended tokens land at
        the end of the S side and shift nothing: ``seq_name`` must be the last configured sequence
        (no [SEP] follows it, model.py:270-272) and present in the requests, and no layer before the
        last may prune (a pyramid keep would move with the length).  Weight groups are functions of the
        absolute position, which the old tokens keep.

        ``seq_fusion='time'``: the stream is ordered by time, so new events of ANY present sequence land at its
        end — when, per request, every time of ``new_times`` ([R, dL] integers) is later than the request's cached
        latest time (``cache.last_time``).  A time equal to it is accepted only for the last configured sequence
        (only there is the tie certain to sort last: the key is (time, sequence, position)).  Checked with one
        small read-back before anything is launched; a violation raises ValueError.  ``new_times`` is ignored
        under 'sep'.

        cache_dtype 'bf16': the new rows go into the layer buffers in place — no copy, the returned cache shares the
        buffers and ``cache`` stays valid — when they fit (``encode_requests(reserve=)``) and ``cache`` ends at the
        buffer's high-water mark; otherwise each layer gets a buffer of max(Ic + dL, 2·cap) rows per request and one
        copy (an old cache extended a second time forks this way)."""
        from .model import _Tokenize
        m = self.m
        cfg = m.config
        d = cfg.hidden_dim
        self._check_cache('extend_requests', cache)
        bf16 = self.cache_dtype == 'bf16'
        seqs = cfg.feature_config['sequence_features']
        if m.time_fusion:
            if seq_name not in seqs or seq_name not in cache.present:
                raise ValueError(f'extend_requests: {seq_name!r} is not a configured sequence present in the cached '
                                 'requests')
        elif seq_name != seqs[-1] or seq_name not in cache.present:
            raise ValueError(f'extend_requests: only the last configured sequence ({seqs[-1]!r}), present in the '
                             'cached requests, can grow without shifting earlier positions')
        old = self.schedule(cache.L_S)
        if any(e['kS'] + e['kN'] < e['I'] for e in old[:-1]):
            raise ValueError('extend_requests: a pyramid keep before the last layer depends on the length; '
                             're-encode instead')
        R = cache.R
        feats = {seq_name: new_events}
        if m.time_fusion:
            feats[seq_name + cfg.seq_time_suffix] = self._check_new_times(cache, seq_name, new_events, new_times)
        if m.padding_mask:
            # appended events are real: their span is all valid, and it attends over the cache under the cache's mask
            if cache.valid is None:
                raise ValueError('extend_requests: the request cache holds no validity (it was not encoded under '
                                 'seq_padding_mask)')
            ev = torch.as_tensor(new_events)
            feats[seq_name + cfg.seq_len_suffix] = np.full(ev.shape[0], ev.shape[1], dtype=np.int32)
        plan = m._plan({}, feats)
        if plan['B'] != R:
            raise ValueError(f'extend_requests: {plan["B"]} rows of new events for {R} cached requests')
        dL = plan['L_S']
        # 'time': the new events among themselves are ordered by the same kernel (one sequence)
        x = s_rows(_Tokenize.apply(m.flat, m, plan), plan)                # [R*dL, d], no [SEP]
        last_time = plan['last_time'].clone() if m.time_fusion else None
        new = self.schedule(cache.L_S + dL)
        req = torch.arange(R, dtype=torch.int32, device=x.device)
        layers = []
        for l, (e_old, e_new) in enumerate(zip(old, new)):
            Ic = e_old['s']
            lay = cache.layers[l]
            keep = e_new['kS'] - e_old['kS']                              # new S rows kept by this layer
            if bf16:
                # the new tokens attend over the bf16 rows and their own f32 rows; then their K/V are appended, in
                # place when the buffer has room behind this cache's rows (the old cache reads only its first Ic)
                x, qkv, _ = span_forward(m, l, x, R, dL, dL if keep == dL else 0, Ic, e_new['I'], cached=True,
                                         kv16=(lay['kv16'], lay['cap']) if Ic > 0 else None, Ic=Ic, req=req, R=R,
                                         valid=_cache_valid(cache.valid, cache.L_S, Ic))
                layers.append(self._kv16_layer(qkv, R, dL, max(Ic + dL, 2 * lay['cap']), Ic, lay))
                continue
            x, qkv, _ = span_forward(m, l, x, R, dL, dL if keep == dL else 0, Ic, e_new['I'], cached=True,
                                     kv=lay['kv'] if Ic > 0 else None, req=req, R=R,
                                     valid=_cache_valid(cache.valid, cache.L_S, Ic))
            kv = qkv if Ic == 0 else torch.cat([lay['kv'].view(R, Ic, 3 * d), qkv.view(R, dL, 3 * d)], 1)
            layers.append({'Ic': Ic + dL, 'kv': kv.reshape(R * (Ic + dL), 3 * d)})
        valid = (torch.cat([cache.valid, torch.ones(R, dL, dtype=torch.uint8, device=m.device)], 1)
                 if m.padding_mask else None)
        return RequestCache(R, cache.L_S + dL, layers, cache.present, last_time, valid, self.cache_dtype)

    def _check_new_times(self, cache: RequestCache, seq_name: str, new_events, new_times) -> torch.Tensor:
        """``extend_requests`` under seq_fusion='time': the new events' times as a device int64 [R, dL] tensor,
        after checking that they sort behind everything cached (one read-back of a flag)."""
        cfg = self.m.config
        if new_times is None:
            raise ValueError(f"extend_requests: seq_fusion='time' needs new_times for {seq_name!r}")
        if cache.last_time is None:
            raise ValueError('extend_requests: the request cache holds no times (it was not encoded under '
                             "seq_fusion='time')")
        t = new_times if isinstance(new_times, torch.Tensor) else torch.as_tensor(new_times)
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f'extend_requests: new_times are {t.dtype}; integer timestamps are expected')
        want = tuple(torch.as_tensor(new_events).shape[:2])
        if tuple(t.shape) != want or t.shape[0] != cache.R or t.shape[1] < 1:
            raise ValueError(f'extend_requests: new_times of {seq_name!r} have shape {tuple(t.shape)}, expected '
                             f'{(cache.R,) + want[1:]}')
        t = t.to(self.m.device, torch.int64)
        first = t.min(dim=1).values
        tie_ok = seq_name == cfg.feature_config['sequence_features'][-1]
        bad = (first < cache.last_time) if tie_ok else (first <= cache.last_time)
        if bool(bad.any()):
            raise ValueError(f'extend_requests: {int(bad.sum())} request(s) have a new {seq_name!r} event '
                             + ('earlier than' if tie_ok else 'not later than')
                             + ' their cached latest event; it would not land at the end of the time-ordered '
                             'stream (re-encode instead)')
        return t

    # ------------------------------------------------------------------ stage II
    def _stage2(self, who: str, cache: RequestCache, req: torch.Tensor, non_seq_features: Dict[str, torch.Tensor]):
        """Candidates' NS tokens (model.py:239-254) through every layer against their request's cache and the
        heads: (probs [T, C], req as device int32 [C])."""
        from .model import _Head, _Tokenize
        m = self.m
        self._check_cache(who, cache)
        bf16 = self.cache_dtype == 'bf16'
        plan = m._plan(non_seq_features, {})
        C = plan['B']
        if m.padding_mask and cache.valid is None:
            raise ValueError(f'{who}: the request cache holds no validity (it was not encoded under seq_padding_mask)')
        check_req(who, req, cache.R, C, ordered=False)
        req = torch.as_tensor(req).to(m.device, torch.int32).contiguous()
        x = _Tokenize.apply(m.flat, m, plan)                              # [C*L_NS, d]: NS tokens only
        for l, e in enumerate(self.schedule(cache.L_S)):
            s, n, kN = e['s'], e['n'], e['kN']
            lay = cache.layers[l]
            if lay['Ic'] != s:
                raise OneTransHipError(f'{who}: request cache does not match the schedule')
            if bf16:
                x, _, _ = span_forward(m, l, x, C, n, kN, s, e['I'], cached=True,
                                       kv16=(lay['kv16'], lay['cap']) if s > 0 else None, Ic=s, req=req, R=cache.R,
                                       valid=_cache_valid(cache.valid, cache.L_S, s))
                continue
            x, _, _ = span_forward(m, l, x, C, n, kN, s, e['I'], cached=True, kv=lay['kv'] if s > 0 else None,
                                   req=req, R=cache.R, valid=_cache_valid(cache.valid, cache.L_S, s))
        probs, _ = _Head.apply(m.flat, x, m)                               # [T, C]
        return probs, req

    @torch.no_grad()
    @K.in_model_precision
    def score(self, cache: RequestCache, req: torch.Tensor, non_seq_features: Dict[str, torch.Tensor]):
        """Stage II for C candidates: returns {task: probs [C, 1]} like ``OneTransModel.forward``
        (model.py:384-391)."""
        probs, _ = self._stage2('score', cache, req, non_seq_features)
        return {t: probs[i].view(-1, 1) for i, t in enumerate(self.m.config.tasks)}

    def _rank_weights(self, weights: Optional[Dict[str, float]]) -> List[float]:
        tasks = list(self.m.config.tasks)
        if weights is None:
            return [1.0] * len(tasks)
        unknown = [t for t in weights if t not in tasks]
        if unknown:
            raise ValueError(f'rank: unknown task(s) {unknown} in weights (the model has {tasks})')
        return [float(weights.get(t, 1.0)) for t in tasks]

    @torch.no_grad()
    @K.in_model_precision
    def rank(self, cache: RequestCache, req: torch.Tensor, non_seq_features: Dict[str, torch.Tensor], k: int,
             weights: Optional[Dict[str, float]] = None, mode: str = 'sum', return_probs: bool = False):
        """Stage II as in ``score``, then per request the ``k`` best of its candidates under one fused score
        (ot_rank_topk on the heads' [T, C] output): ``mode`` 'sum' ranks by Σ_task w·p, 'product' by Π_task p over
        the tasks whose weight is not 0 (pCTR · pCVR).  ``weights`` {task: float}, default 1 for every task.
        Equal scores go to the lower candidate index.  Returns device tensors, no host sync:
        'index' int32 [R, k] (positions in this call's candidate batch, -1 past 'count'), 'score' f32 [R, k]
        (-inf past 'count'), 'count' int32 [R] = min(k, the request's candidates); with ``return_probs`` also
        'probs' {task: [C, 1]} as ``score`` returns."""
        from ._lib import RANK_MAX_K, RANK_MODES
        k = int(k)
        if k < 1 or k > RANK_MAX_K:
            raise ValueError(f'rank: k={k} out of range (1..{RANK_MAX_K})')
        if mode not in RANK_MODES:
            raise ValueError(f'rank: mode {mode!r}, expected one of {sorted(RANK_MODES)}')
        w = self._rank_weights(weights)
        probs, req = self._stage2('rank', cache, req, non_seq_features)
        T, C = probs.shape
        R, dev = cache.R, probs.device
        out = {'index': torch.empty(R, k, dtype=torch.int32, device=dev),
               'score': torch.empty(R, k, dtype=torch.float32, device=dev),
               'count': torch.empty(R, dtype=torch.int32, device=dev)}
        K.rank_topk(probs, probs.stride(0), T, w, mode, req, C, R, k, out['index'], out['score'], out['count'],
                    device=dev)
        if return_probs:
            out['probs'] = {t: probs[i].view(-1, 1) for i, t in enumerate(self.m.config.tasks)}
        return out

    @torch.no_grad()
    @K.in_model_precision
    def predict(self, non_seq_features, seq_features, req: Optional[torch.Tensor] = None):
        """One call: ``seq_features`` hold R requests, ``non_seq_features`` C candidates, ``req`` [C] maps
        candidates to requests (default: candidate i belongs to request i, R == C)."""
        cache = self.encode_requests(seq_features)
        if req is None:
            req = torch.arange(cache.R, dtype=torch.int32)
        return self.score(cache, req, non_seq_features)


class OneTransInferenceEngine:
    """The reference's inference engine surface (examples/inference_example.py:21-219): load a saved
    model directory (config.json + weights, train.py:281-291), preprocess, single / batch inference,
    latency statistics.  ``score_candidates`` adds the two-stage path: one user's sequences once,
    many candidates against the cache (``cache_dtype`` 'fp32' or 'bf16': ``OneTransServer``'s request cache)."""

    def __init__(self, model_path: str, device=None, cache_dtype: str = 'fp32'):
        import json
        import os
        from .config import OneTransConfig
        from .model import OneTransModel
        cfg_path = os.path.join(model_path, 'config.json')
        if not os.path.exists(cfg_path):                                  # inference_example.py:44-45
            raise FileNotFoundError(f'config file not found: {cfg_path}')
        with open(cfg_path) as f:
            self.config = OneTransConfig.from_dict(json.load(f))
        w = os.path.join(model_path, 'model_weights.npz')
        if not os.path.exists(w):                                          # inference_example.py:55-56
            raise FileNotFoundError(f'model weights not found: {w}')
        self.model = OneTransModel(self.config, device=device)
        self.model.load_weights(w)
        self.server = OneTransServer(self.model, cache_dtype)      # 'bf16': score_candidates / rank_candidates
        self.reset_stats()

    # ------------------------------------------------------------------ inference_example.py:63-92
    def preprocess_input(self, user_features: Dict, item_features: Dict, context_features: Dict,
                         sequence_features: Dict):
        from .features import SequenceProcessor
        import numpy as np
        non_seq = {}
        non_seq.update(user_features)
        non_seq.update(item_features)
        non_seq.update(context_features)
        sp = SequenceProcessor(self.config)
        # a sequence's companion times (name + seq_time_suffix) are left-padded with INT64_MIN, not zeros: padding
        # events sort first in the time-ordered stream
        seq = {k: sp.process_times(v) if sp.is_time_key(k, sequence_features) else sp.process_sequence(np.asarray(v))
               for k, v in sequence_features.items()}
        if getattr(self.config, 'seq_padding_mask', False):
            # variable-length histories: the number of real events process_sequence kept (the last ``len`` positions)
            seq.update({k + sp.len_suffix: sp.lengths([np.asarray(v)])[0] for k, v in sequence_features.items()
                        if not sp.is_time_key(k, sequence_features)})
        return non_seq, seq

    def _is_bag(self, name: str) -> bool:
        bags = getattr(self.config, 'bag_features', None) or {}
        return name in bags or (name.endswith('_weight') and name[:-len('_weight')] in bags)

    def _ns_tensor(self, name: str, v, dev):
        """One NS input on the device: [B, 1], or a bag feature's padded [B, cap] ids / weights as they are."""
        import numpy as np
        if self._is_bag(name):
            t = torch.as_tensor(np.asarray(v))
            if t.dim() != 2:                           # one sample's Python list of ids (or of weights)
                from .features import FeatureProcessor
                t = (torch.from_numpy(FeatureProcessor.pad_bags([v])) if name in self.config.bag_features
                     else t.to(torch.float32).reshape(1, -1))
            return t.to(dev)
        return torch.as_tensor(np.asarray(v)).reshape(-1, 1).to(dev)

    def _predict(self, non_seq, seq):
        import numpy as np
        dev = self.model.device
        ns = {k: self._ns_tensor(k, v, dev) for k, v in non_seq.items()}
        sq = {k: torch.as_tensor(np.asarray(v)).to(dev) for k, v in seq.items()}
        with torch.no_grad():
            out = self.model((ns, sq), training=False)
        return {t: p.float().cpu().numpy()[:, 0] for t, p in out.items()}

    def single_inference(self, user_features, item_features, context_features, sequence_features) -> Dict[str, float]:
        """inference_example.py:94-129."""
        import time
        t0 = time.time()
        try:
            ns, seq = self.preprocess_input(user_features, item_features, context_features, sequence_features)
            seq = {k: v[None] for k, v in seq.items()}                     # batch dimension
            res = {t: float(v[0]) for t, v in self._predict(ns, seq).items()}
            self._update_stats(True, (time.time() - t0) * 1e3)
            return res
        except Exception:
            self._update_stats(False, 0.0)
            raise

    def batch_inference(self, batch_data) -> List[Dict[str, float]]:
        """inference_example.py:131-179: (user, item, context, sequences) tuples, one full forward."""
        import time
        import numpy as np
        t0 = time.time()
        try:
            pre = [self.preprocess_input(*b) for b in batch_data]
            from .features import FeatureProcessor
            bags = getattr(self.config, 'bag_features', None) or {}
            ns = {k: (FeatureProcessor.pad_bags([p[0][k] for p in pre]) if k in bags
                      else np.concatenate([np.asarray(p[0][k]).reshape(-1) for p in pre])) for k in pre[0][0]}
            seq = {k: np.stack([p[1][k] for p in pre]) for k in pre[0][1]}
            out = self._predict(ns, seq)
            n = len(batch_data)
            self._update_stats(True, (time.time() - t0) * 1e3 / n, n)
            return [{t: float(v[i]) for t, v in out.items()} for i in range(n)]
        except Exception:
            self._update_stats(False, 0.0, len(batch_data))
            raise

    def _one_request(self, user_features: Dict, sequence_features: Dict, candidates: List[Dict]):
        """Stage I for one request and its candidates' NS features on the device: (cache, features)."""
        import numpy as np
        dev = self.model.device
        _, seq = self.preprocess_input({}, {}, {}, sequence_features)
        cache = self.server.encode_requests({k: torch.as_tensor(v[None]).to(dev) for k, v in seq.items()})
        ns = {}
        from .features import FeatureProcessor
        bags = getattr(self.config, 'bag_features', None) or {}
        C = len(candidates)
        for k, v in user_features.items():
            if k in bags:                              # a request-level bag: one id list, shared by the candidates
                ns[k] = np.repeat(FeatureProcessor.pad_bags([v]), C, axis=0)
            else:
                ns[k] = np.repeat(np.asarray(v).reshape(-1)[:1], C)
        for k in candidates[0]:
            if k in bags:                              # a candidate-level bag: each candidate's Python list of ids
                ns[k] = FeatureProcessor.pad_bags([c[k] for c in candidates])
            elif self._is_bag(k):                      # its per-slot weights, padded like the ids (tail kept)
                cap = max([len(c[k]) for c in candidates] + [1])
                w = np.zeros((C, cap), dtype=np.float32)
                for i, c in enumerate(candidates):
                    if len(c[k]):
                        w[i, :len(c[k])] = np.asarray(c[k], dtype=np.float32)
                ns[k] = w
            else:
                ns[k] = np.concatenate([np.asarray(c[k]).reshape(-1) for c in candidates])
        return cache, {k: self._ns_tensor(k, v, dev) for k, v in ns.items()}

    def score_candidates(self, user_features: Dict, sequence_features: Dict, candidates: List[Dict]):
        """One request (user + sequences), many candidates (item / context features each): stage I once,
        stage II for all candidates (paper §3.5.1).  Same results as ``batch_inference`` on the
        (user, candidate, sequences) samples."""
        cache, nsd = self._one_request(user_features, sequence_features, candidates)
        out = self.server.score(cache, torch.zeros(len(candidates), dtype=torch.int32), nsd)
        return [{t: float(p[i, 0]) for t, p in out.items()} for i in range(len(candidates))]

    def rank_candidates(self, user_features: Dict, sequence_features: Dict, candidates: List[Dict], k: int,
                        weights: Optional[Dict[str, float]] = None, mode: str = 'sum'):
        """``score_candidates``' path, then the ``k`` best candidates under the fused score (``OneTransServer.rank``):
        a list of (candidate index, fused score, {task: prob}) in rank order, min(k, len(candidates)) long.  Only
        the winners come back: their indices, scores and per-task probabilities are gathered on the device and
        copied to the host in one transfer."""
        import time
        t0 = time.time()
        try:
            cache, nsd = self._one_request(user_features, sequence_features, candidates)
            C = len(candidates)
            out = self.server.rank(cache, torch.zeros(C, dtype=torch.int32), nsd, k, weights=weights, mode=mode,
                                   return_probs=True)
            n = min(int(k), C)                                             # one request holding every candidate
            idx = out['index'][0, :n]
            tasks = list(self.config.tasks)
            won = torch.stack([out['probs'][t][:, 0] for t in tasks])[:, idx.long()]          # [T, n]
            packed = torch.cat([idx.view(1, n), out['score'][0, :n].view(torch.int32).view(1, n),
                                won.view(torch.int32)]).cpu().numpy()                          # the one copy
            score, probs = packed[1].view('float32'), packed[2:].view('float32')
            res = [(int(packed[0, j]), float(score[j]), {t: float(probs[i, j]) for i, t in enumerate(tasks)})
                   for j in range(n)]
            self._update_stats(True, (time.time() - t0) * 1e3)
            return res
        except Exception:
            self._update_stats(False, 0.0)
            raise

    # ------------------------------------------------------------------ inference_example.py:181-219
    def _update_stats(self, success: bool, latency: float, batch_size: int = 1):
        st = self.inference_stats
        st['total_requests'] += batch_size
        if success:
            st['successful_requests'] += batch_size
            st['avg_latency_ms'] = 0.1 * latency + 0.9 * st['avg_latency_ms']      # EMA, alpha 0.1
        else:
            st['failed_requests'] += batch_size

    def get_stats(self) -> Dict:
        st = dict(self.inference_stats)
        st['success_rate'] = (st['successful_requests'] / st['total_requests'] * 100
                              if st['successful_requests'] > 0 else 0.0)
        return st

    def reset_stats(self):
        self.inference_stats = {'total_requests': 0, 'avg_latency_ms': 0.0, 'successful_requests': 0,
                                'failed_requests': 0}
