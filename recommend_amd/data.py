"""Synthetic input batches (SURVEY §8d "Synthetic inputs").

* ``create_sample_batch`` — the reference's input contract
  (``data_loader.py:301-329``): user features int U[0,100), item features int
  U[0,1000), context features float U[0,1), each ``[B,1]``; every sequence
  ``[B, L_i, 64]`` U[0,1).  Differences, all recorded in DESIGN.md: the NS
  ints are returned as float32 (defect D3: the reference concatenates int32 with
  float32 at ``model.py:253``), the sequence lengths are given instead of drawn
  per call (``data_loader.py:319``), and labels are Bernoulli draws from a fixed
  teacher instead of uniform floats (defect D7, ``data_loader.py:327``).
* ``criteo_batch`` — the Criteo-shape workload of BASELINE.json configs 2-5:
  13 dense floats ``log1p(lognormal(0,1))``, 26 categorical ids
  ``Zipf(1.1) mod cardinality`` and 3 item-id sequences.

* ``seq_times`` — when ``config.seq_fusion == 'time'`` both generators also emit each sequence's event times
  (``name + config.seq_time_suffix``, int64 ``[B, L_i]``) from a generator of their own, so every other array of a
  batch is bit-identical to the ``'sep'`` batch of the same seed.

* ``bag_ids`` — when ``config.bag_features`` is set, ``criteo_batch`` also emits each bag feature's padded ids
  (int64 ``[B, cap]``, ``-1`` = empty slot; Zipf ids, lengths from 0 to cap) and, for every other 'sum' bag,
  per-slot weights ``name + '_weight'``; again from a generator of their own.

* ``ragged_lengths`` — history lengths for ``config.seq_padding_mask`` (``name + config.seq_len_suffix``, int32
  ``[B]``; empty and full histories both occur), for tests and tools/padmask_bench.py.  ``make_batch`` itself emits none.

* ``gate_task_weights`` / ``downsample_negatives`` — host helpers for ``config.weighted_loss``: a task weight gated
  on another task's label (conversion labels exist on clicked impressions only), and negative down-sampling with the
  kept negatives re-weighted by ``1 / keep_rate``.

All generators are numpy ``Generator(PCG64)``: same seed => same batch, here and
on the GPU box.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from .config import OneTransConfig

Batch = Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray], Dict[str, np.ndarray]]


def _teacher_labels(rng_seed: int, B: int, tasks: List[str], signal: np.ndarray) -> Dict[str, np.ndarray]:
    """Bernoulli(sigmoid(teacher logit)); the teacher is a fixed function of the inputs
    (seed 7) so AUC after training is meaningful (> 0.5)."""
    rng = np.random.Generator(np.random.PCG64(rng_seed))
    labels = {}
    for ti, t in enumerate(tasks):
        z = signal[:, ti % signal.shape[1]]
        p = 1.0 / (1.0 + np.exp(-z))
        labels[t] = (rng.random(B) < p).astype(np.float32).reshape(B, 1)
    return labels


TIME_ORIGIN = 1_700_000_000        # epoch seconds of the synthetic event times


def seq_times(seed: int, B: int, names: List[str], lens: List[int], suffix: str = '_time') -> Dict[str, np.ndarray]:
    """Synthetic event times for ``seq_fusion='time'``: {name + suffix: int64 [B, L]} epoch seconds.  Each
    sequence ascends in time except for a few swapped neighbours (real logs arrive slightly out of order), and
    all sequences draw from one short span, so times tie within and across sequences.  The generator is its own
    (seeded by ``seed``): the other arrays of a batch do not depend on whether times are drawn."""
    rng = np.random.Generator(np.random.PCG64([int(seed), 0x74696D65]))
    span = max(4, 2 * int(sum(lens)))
    rows = np.arange(B)
    out = {}
    for name, L in zip(names, lens):
        t = np.sort(rng.integers(0, span, size=(B, L)), axis=1)
        for _ in range(max(1, L // 16) if L >= 2 else 0):
            i = rng.integers(0, L - 1, size=B)
            t[rows, i], t[rows, i + 1] = t[rows, i + 1].copy(), t[rows, i].copy()
        out[name + suffix] = (TIME_ORIGIN + t).astype(np.int64)
    return out


def ragged_lengths(B: int, config: OneTransConfig, seed: int = 1000, mean_fill: float = 0.5,
                   seq_lens: Optional[List[int]] = None) -> Dict[str, np.ndarray]:
    """Synthetic history lengths for ``seq_padding_mask``: {name + config.seq_len_suffix: int32 [B]} for every
    configured sequence, binomial with mean ``mean_fill`` * L_name.  Sample 0 has empty histories and sample 1 (if any)
    full ones; a generator of its own (seeded by ``seed``), so ``make_batch``'s arrays do not depend on it.  The real
    events are the last ``len`` positions of ``make_batch``'s (full-length) sequences; what sits before them is padding
    content, which the masked model must ignore."""
    rng = np.random.Generator(np.random.PCG64([int(seed), 0x6C656E]))
    names = config.feature_config['sequence_features']
    caps = seq_lens or getattr(config, '_seq_lens', None) or [10] * len(names)
    out = {}
    for name, L in zip(names, caps):
        lens = rng.binomial(int(L), min(1.0, max(0.0, float(mean_fill))), size=B)
        if B > 0:
            lens[0] = 0
        if B > 1:
            lens[1] = L
        out[name + config.seq_len_suffix] = lens.astype(np.int32)
    return out


BAG_CAP = 8                         # default slots per sample of the synthetic bag features


def bag_ids(seed: int, B: int, rows: int, cap: int, mean_fill: float = None) -> np.ndarray:
    """One bag feature's padded ids: int64 [B, cap], sample b's first len_b slots hold ``Zipf(1.1) mod rows`` ids
    (repeats inside a bag happen), the rest -1.  The lengths are binomial with mean ``mean_fill`` (default cap / 2),
    so empty and full bags both occur; sample 0 is always empty and sample 1 (if any) full."""
    rng = np.random.Generator(np.random.PCG64([int(seed), 0x626167]))
    fill = cap / 2.0 if mean_fill is None else float(mean_fill)
    lens = rng.binomial(cap, min(1.0, max(0.0, fill / cap)), size=B)
    lens[0] = 0
    if B > 1:
        lens[1] = cap
    ids = (rng.zipf(1.1, size=(B, cap)) - 1) % int(rows)
    return np.where(np.arange(cap)[None, :] < lens[:, None], ids, -1).astype(np.int64)


def _add_bags(ns: Dict[str, np.ndarray], config: OneTransConfig, seed: int, B: int, bags=None) -> None:
    """``bags``: None (every configured bag feature, BAG_CAP slots), or {name: cap} / {name: (cap, mean fill)}."""
    cfgd = getattr(config, 'bag_features', None) or {}
    if not cfgd:
        return
    spec = {n: BAG_CAP for n in cfgd} if bags is None else dict(bags)
    k = 0
    for name in config.ns_feature_names():
        if name not in cfgd or name not in spec:
            continue
        cap, fill = spec[name] if isinstance(spec[name], (tuple, list)) else (spec[name], None)
        ns[name] = bag_ids(seed * 131 + k, B, config.bag_rows(name), int(cap), fill)
        if config.bag_pooling(name) == 'sum' and k % 2 == 0:
            wrng = np.random.Generator(np.random.PCG64([int(seed), 0x776774, k]))
            ns[name + '_weight'] = wrng.uniform(0.25, 2.0, size=ns[name].shape).astype(np.float32)
        k += 1


def _add_times(seq: Dict[str, np.ndarray], config: OneTransConfig, seed: int) -> None:
    if getattr(config, 'seq_fusion', 'sep') != 'time' or not seq:
        return
    B = next(iter(seq.values())).shape[0]
    seq.update(seq_times(seed, B, list(seq), [v.shape[1] for v in seq.values()], config.seq_time_suffix))


def create_sample_batch(batch_size: int, config: OneTransConfig, seq_lens: Optional[List[int]] = None,
                        seed: int = 1000) -> Batch:
    """data_loader.py:301-329 with the deviations listed in the module docstring."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B = batch_size
    fc = config.feature_config
    ns: Dict[str, np.ndarray] = {}
    for name in fc['user_features']:
        ns[name] = rng.integers(0, 100, size=(B, 1)).astype(np.float32)
    for name in fc['item_features']:
        ns[name] = rng.integers(0, 1000, size=(B, 1)).astype(np.float32)
    for name in fc['context_features']:
        ns[name] = rng.random((B, 1), dtype=np.float32)
    seq: Dict[str, np.ndarray] = {}
    lens = seq_lens or getattr(config, '_seq_lens', None) or [10] * len(fc['sequence_features'])
    for name, L in zip(fc['sequence_features'], lens):
        seq[name] = rng.random((B, L, config.seq_feature_dim), dtype=np.float32)
    _add_times(seq, config, seed)
    trng = np.random.Generator(np.random.PCG64(7))
    nsmat = np.concatenate([ns[n] for n in config.ns_feature_names() if n in ns], axis=1)
    a = trng.normal(size=(nsmat.shape[1], 2)) / np.sqrt(nsmat.shape[1])
    z = (nsmat / np.maximum(nsmat.max(axis=0, keepdims=True), 1.0)) @ a
    z = 3.0 * (z - z.mean(axis=0))
    labels = _teacher_labels(seed + 1, B, config.tasks, z)
    return ns, seq, labels


def criteo_batch(batch_size: int, config: OneTransConfig, seq_lens: Optional[List[int]] = None,
                 seed: int = 1000, teacher: str = 'ids', bags=None) -> Batch:
    """Criteo-shape batch: dense I* float32 [B,1]; sparse C* int64 [B,1]; seqs int64 [B,L_i]; the bag features of
    ``config.bag_features`` int64 [B, cap] padded with -1 (``bags``: {name: cap} or {name: (cap, mean fill)};
    default every bag feature with BAG_CAP slots; they do not enter the label signal).

    ``teacher`` picks the label signal: 'ids' (default; every feature, the sparse ids through a hashed
    per-id effect — learnable only by memorising ids) or 'dense' (the 13 dense features alone, 4x the
    weight: a signal a few hundred steps of training pick up, for tests that need a model that has
    learned)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B = batch_size
    fc = config.feature_config
    ns: Dict[str, np.ndarray] = {}
    trng = np.random.Generator(np.random.PCG64(7))
    signal = np.zeros((B, 2))
    dense_signal = np.zeros((B, 2))
    for name in config.ns_feature_names():
        if name in (getattr(config, 'bag_features', None) or {}):
            continue                                   # drawn below, from a generator of their own
        if name in config.sparse_features:
            card = config.sparse_features[name]
            ids = (rng.zipf(1.1, size=(B, 1)) - 1) % card
            ns[name] = ids.astype(np.int64)
            u = trng.normal(size=(1024, 2)) * 0.3
            signal += u[(ids[:, 0] * 2654435761) % 1024]
        else:
            v = np.log1p(rng.lognormal(0.0, 1.0, size=(B, 1))).astype(np.float32)
            ns[name] = v
            w = trng.normal(size=(1, 2)) * 0.3
            signal += v * w
            dense_signal += v * w * 4.0
    seq: Dict[str, np.ndarray] = {}
    lens = seq_lens or getattr(config, '_seq_lens', None)
    vocab = config.seq_item_vocab
    for name, L in zip(fc['sequence_features'], lens):
        seq[name] = ((rng.zipf(1.1, size=(B, L)) - 1) % vocab).astype(np.int64)
    _add_times(seq, config, seed)
    _add_bags(ns, config, seed, B, bags)
    if teacher == 'dense':
        signal = dense_signal
    elif teacher != 'ids':
        raise ValueError(f"teacher {teacher!r}: 'ids' or 'dense'")
    labels = _teacher_labels(seed + 1, B, config.tasks, signal - signal.mean(axis=0))
    return ns, seq, labels


def make_batch(batch_size: int, config: OneTransConfig, seed: int = 1000,
               seq_lens: Optional[List[int]] = None, teacher: str = 'ids') -> Batch:
    """Dispatch on the config: Criteo-shape when embedding tables are configured (``teacher``: criteo_batch)."""
    if config.sparse_features or config.seq_item_vocab:
        return criteo_batch(batch_size, config, seq_lens, seed, teacher)
    return create_sample_batch(batch_size, config, seq_lens, seed)


RequestBatch = Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray], Dict[str, np.ndarray], np.ndarray]


def make_request_batch(R: int, cands, config: OneTransConfig, seed: int = 1000,
                       seq_lens: Optional[List[int]] = None, teacher: str = 'ids') -> RequestBatch:
    """A request-grouped batch ``(non_seq, seq, labels, req)``: R requests' sequences (and, for
    ``seq_fusion='time'``, their ``*_time`` arrays) with R rows, C candidates' non-sequence features and labels
    with C rows, and ``req`` int32 [C], non-decreasing: the request of each candidate.  ``cands``: candidates
    per request, an int or a list of R counts (zeros allowed).  The candidate side is ``make_batch(C, seed)``'s,
    the request side ``make_batch(R, seed + 1)``'s sequences."""
    counts = [int(cands)] * R if np.isscalar(cands) else [int(c) for c in cands]
    if len(counts) != R or any(c < 0 for c in counts):
        raise ValueError(f'cands: {R} non-negative counts expected, got {counts}')
    C = sum(counts)
    ns, _, labels = make_batch(C, config, seed, seq_lens, teacher)
    _, seq, _ = make_batch(R, config, seed + 1, seq_lens, teacher)
    req = np.repeat(np.arange(R, dtype=np.int32), counts)
    return ns, seq, labels, req


def expand_requests(batch: RequestBatch) -> Batch:
    """The per-sample 3-tuple equal to a request-grouped batch: every sequence array (``*_time`` included)
    gathered by ``req``, so candidate c carries a copy of its request's sequences."""
    ns, seq, labels, req = batch
    idx = np.asarray(req, dtype=np.int64)
    return ns, {k: np.asarray(v)[idx] for k, v in seq.items()}, labels


def gate_task_weights(labels: Dict[str, np.ndarray], task: str = 'cvr', gate: str = 'ctr',
                      suffix: str = '_weight') -> Dict[str, np.ndarray]:
    """A copy of ``labels`` with ``labels[task + suffix]`` = 1 where ``labels[gate] > 0.5`` and 0 elsewhere (float32,
    the gate's shape): under ``config.weighted_loss`` task ``task`` then trains and is measured on the gated rows
    only — a CVR head on clicked impressions — and its label elsewhere is never read (it may be NaN)."""
    if task not in labels or gate not in labels:
        raise KeyError(f'gate_task_weights: labels hold {sorted(labels)}, not both {task!r} and {gate!r}')
    out = dict(labels)
    out[task + suffix] = (np.asarray(labels[gate]) > 0.5).astype(np.float32)
    return out


def downsample_negatives(batch, task: str, keep_rate: float, seed: int, weight_key: str = 'sample_weight'):
    """Negative down-sampling of a host batch: every row whose ``labels[task]`` is not > 0.5 is kept with probability
    ``keep_rate`` (numpy PCG64 of ``seed``), every positive is kept; ``labels[weight_key]`` of the result is
    ``1 / keep_rate`` on the kept negatives and 1 on the positives (times the batch's own weight, if it has one), so
    the weighted loss and metrics estimate those of the full stream.  Every array of ``non_seq``, ``seq`` and
    ``labels`` is cut to the kept rows; in a request-grouped 4-tuple the candidate side (``non_seq``, ``labels``,
    ``req``) is cut and the request side stays."""
    if not 0.0 < float(keep_rate) <= 1.0:
        raise ValueError(f'downsample_negatives: keep_rate {keep_rate!r} not in (0, 1]')
    ns, seq, labels = batch[0], batch[1], batch[2]
    y = np.asarray(labels[task]).reshape(-1)
    rng = np.random.Generator(np.random.PCG64([int(seed), 0x6E6567]))
    neg = ~(y > 0.5)
    keep = ~neg | (rng.random(len(y)) < float(keep_rate))
    rows = np.nonzero(keep)[0]
    cut = lambda d: {k: np.asarray(v)[rows] for k, v in d.items()}
    lab = cut(labels)
    shape = np.asarray(labels[task]).shape
    w = np.where(neg, np.float32(1.0 / float(keep_rate)), np.float32(1.0)).astype(np.float32).reshape(shape)[rows]
    if weight_key in labels:
        w = (w.reshape(-1) * np.asarray(labels[weight_key], dtype=np.float32).reshape(-1)[rows]).reshape(w.shape)
    lab[weight_key] = w.astype(np.float32)
    if len(batch) == 4:
        return cut(ns), dict(seq), lab, np.asarray(batch[3])[rows]
    return cut(ns), cut(seq), lab
