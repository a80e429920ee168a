"""Evaluation metrics of the reference trainer/evaluator.

* ``auc`` — exact rank-based ROC AUC (Mann-Whitney U, average ranks for ties): the primary
  parity estimator, identical on both sides.
* ``keras_auc`` — ``tf.keras.metrics.AUC()`` defaults (train.py:101, evaluate.py:45): ROC over 200
  thresholds, trapezoidal interpolation.
* ``uauc`` — the paper's second offline metric, the impression-weighted user-level AUC
  (complete_translation.md:178-180): the rank AUC inside each group (user), averaged with the groups'
  impression counts as weights.
All three are host-side numpy over whole arrays of probabilities.
* ``GroupedAUC`` — ``uauc`` as a device-side metric: a device log of (group, label, probability) records,
  appended to without a host sync, and one ``ot_grouped_auc`` call (sort + segmented rank statistic) per read.
* ``StreamingMetrics`` — the reference's running per-step metrics (AUC, BinaryAccuracy, Precision, Recall; MSE,
  MAE; logloss and F1 for the evaluator) as device state: one HIP launch per step (``ot_metrics_update``), no
  host sync, read once per epoch.
"""

from __future__ import annotations

from typing import Dict

import numpy as np


def _weighted_auc(y, s, w) -> float:
    """Σ_{pos i, neg j} w_i w_j ([s_i > s_j] + [s_i == s_j] / 2) / (W_pos W_neg): the Mann-Whitney statistic of the
    records replicated w times (for integer w exactly that).  Zero-weight records are dropped first, whatever
    they hold; without weight in one of the classes the result is NaN, as un-weighted."""
    keep = w > 0
    y, s, w = y[keep], s[keep], w[keep]
    pos = y > 0.5
    wp, wn = np.where(pos, w, 0.0), np.where(pos, 0.0, w)
    if wp.sum() == 0 or wn.sum() == 0:
        return float('nan')
    order = np.argsort(s, kind='mergesort')
    ss, wp, wn = s[order], wp[order], wn[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(ss))[0] + 1])            # tie runs
    gp, gn = np.add.reduceat(wp, starts), np.add.reduceat(wn, starts)
    below = np.cumsum(gn) - gn                                                # negative weight strictly below the run
    return float(np.sum(gp * (below + 0.5 * gn)) / (wp.sum() * wn.sum()))


def _weights_arg(weights, n: int) -> np.ndarray:
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != n:
        raise ValueError(f'weights: {n} values expected, got {len(w)}')
    if not bool(np.all(w >= 0)):
        raise ValueError('weights must be >= 0 (no NaN)')
    return w


def auc(labels, scores, weights=None) -> float:
    """``weights`` ([n], >= 0): the weighted statistic (``_weighted_auc``); None: every record counts once."""
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if weights is not None:
        return _weighted_auc(y, s, _weights_arg(weights, len(s)))
    order = np.argsort(s, kind='mergesort')
    ss = s[order]
    n = len(s)
    # average ranks for ties
    ranks = np.empty(n)
    boundaries = np.nonzero(np.diff(ss))[0] + 1
    starts = np.concatenate([[0], boundaries])
    ends = np.concatenate([boundaries, [n]])
    for a, b in zip(starts, ends):
        ranks[order[a:b]] = 0.5 * (a + b - 1) + 1.0
    pos = y > 0.5
    npos, nneg = pos.sum(), n - pos.sum()
    if npos == 0 or nneg == 0:
        return float('nan')
    return float((ranks[pos].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


def keras_thresholds(num_thresholds: int = 200) -> np.ndarray:
    """``tf.keras.metrics.AUC(num_thresholds)``'s thresholds: -eps, i/(n-1) for i = 1..n-2, 1+eps."""
    eps = 1e-7
    return np.array([0.0 - eps] + [(i + 1) / (num_thresholds - 1) for i in range(num_thresholds - 2)] + [1.0 + eps])


def div_no_nan(a, b):
    """``tf.math.divide_no_nan`` in float64: 0 where the denominator is 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape), where=b > 0)


def roc_trapezoid(tp, fp, P, N) -> float:
    """Keras's ROC AUC ('interpolation' summation) from the true / false positives at each threshold
    (ascending thresholds) and the class totals ``P``, ``N``: shared by ``keras_auc`` and ``StreamingMetrics``."""
    fn, tn = P - tp, N - fp
    rec = np.divide(tp, tp + fn, out=np.zeros(len(tp)), where=(tp + fn) > 0)
    fpr = np.divide(fp, fp + tn, out=np.zeros(len(tp)), where=(fp + tn) > 0)
    return float(np.sum((fpr[:-1] - fpr[1:]) * (rec[:-1] + rec[1:]) / 2.0))


def keras_auc(labels, probs, num_thresholds: int = 200, weights=None) -> float:
    """``weights`` ([n], >= 0): Keras's ``sample_weight`` — the true / false positives at each threshold are sums of
    weights; zero-weight records are dropped first, whatever they hold."""
    thr = keras_thresholds(num_thresholds)
    y = np.asarray(labels).reshape(-1) > 0.5
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    if weights is not None:
        w = _weights_arg(weights, len(p))
        keep = w > 0
        y, p, w = y[keep], p[keep], w[keep]
        order = np.argsort(p, kind='mergesort')
        ps, ys, ws_ = p[order], y[order], w[order]
        at = np.searchsorted(ps, thr, side='right')                          # the records > thr are ps[at:]
        cp = np.concatenate([[0.0], np.cumsum(np.where(ys, ws_, 0.0))])
        cn = np.concatenate([[0.0], np.cumsum(np.where(ys, 0.0, ws_))])
        return roc_trapezoid(cp[-1] - cp[at], cn[-1] - cn[at], cp[-1], cn[-1])
    ps = np.sort(p)
    # counts of predictions > thr via searchsorted (O(n log n))
    gt = len(p) - np.searchsorted(ps, thr, side='right')
    pos_sorted = np.sort(p[y])
    tp = len(pos_sorted) - np.searchsorted(pos_sorted, thr, side='right')
    fp = gt - tp
    return roc_trapezoid(tp, fp, y.sum(), (~y).sum())


def _orderable(scores) -> np.ndarray:
    """f32 scores -> uint32 keys in the same order, under the rules of ``ot_grouped_auc``: -0.0 ties with +0.0,
    every NaN ties with every other NaN and ranks above +inf."""
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1))
    u = s.view(np.uint32).copy()
    u[s == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    u = np.where(neg, ~u, u | np.uint32(0x80000000))
    u[np.isnan(s)] = 0xFFFFFFFF
    return u


def uauc(groups, labels, scores) -> Dict:
    """Impression-weighted group-level AUC of one binary task (the definition of ``ot_grouped_auc``, in float64
    numpy): per distinct group u the class counts and the exact integer 2U = Σ_{pos p, neg q} (2·[s_p > s_q] +
    [s_p == s_q]); a group is valid with both classes present, AUC_u = 2U / (2·n_pos·n_neg);
    ``uauc`` = Σ_valid n_u·AUC_u / Σ_valid n_u (0 without a valid group, ``div_no_nan``).  Also ``uauc_macro`` (the
    plain mean over valid groups), ``users`` and ``impressions`` (the valid groups and their records), and per
    distinct group, ascending as unsigned 64-bit ids: ``groups`` [G] int64 and ``group_stats`` [G, 3] int64
    {n_pos, n_neg, 2U}.  Scores are compared as float32: -0.0 ties with +0.0, NaNs tie with each other above +inf."""
    g = np.ascontiguousarray(np.asarray(groups).reshape(-1).astype(np.int64)).view(np.uint64)
    pos = np.asarray(labels).reshape(-1) > 0.5
    key = _orderable(scores)
    n = len(g)
    if not (len(pos) == n and len(key) == n):
        raise ValueError('uauc: groups, labels and scores must have the same number of records')
    if n == 0:
        return {'uauc': 0.0, 'uauc_macro': 0.0, 'users': 0, 'impressions': 0,
                'groups': np.zeros(0, np.int64), 'group_stats': np.zeros((0, 3), np.int64)}
    ids, dense = np.unique(g, return_inverse=True)
    full = (dense.reshape(-1).astype(np.uint64) << np.uint64(32)) | key.astype(np.uint64)
    order = np.argsort(full, kind='stable')
    ks, ps = full[order], pos[order]
    seg = np.concatenate([[0], np.cumsum(np.bincount(dense.reshape(-1), minlength=len(ids)))]).astype(np.int64)
    head = np.concatenate([[True], ks[1:] != ks[:-1]])                          # tie-run heads
    starts = np.nonzero(head)[0].astype(np.int64)
    ends = np.concatenate([starts[1:], [n]]).astype(np.int64)
    run = np.cumsum(head) - 1
    twice_rank = starts[run] + ends[run] + 1 - 2 * seg[(ks >> np.uint64(32)).astype(np.int64)]
    npos = np.add.reduceat(ps.astype(np.int64), seg[:-1])
    nneg = np.diff(seg) - npos
    u2 = np.add.reduceat(np.where(ps, twice_rank, 0).astype(np.int64), seg[:-1]) - npos * (npos + 1)
    valid = (npos > 0) & (nneg > 0)
    au = u2[valid].astype(np.float64) / (2.0 * npos[valid].astype(np.float64) * nneg[valid].astype(np.float64))
    nu = (npos + nneg)[valid].astype(np.float64)
    return {'uauc': float(div_no_nan(np.sum(nu * au), np.sum(nu))),
            'uauc_macro': float(div_no_nan(np.sum(au), float(valid.sum()))),
            'users': int(valid.sum()), 'impressions': int(nu.sum()),
            'groups': ids.view(np.int64), 'group_stats': np.stack([npos, nneg, u2], axis=1)}


class StreamingMetrics:
    """The reference's running Keras metrics (train.py:95-109, evaluate.py:39-56) as additive device state.

    ``counts`` [T, 2, nb+1] int64: per task and label class (``label > 0.5``), a histogram of the probabilities
    over ``bounds`` — the ``num_thresholds`` Keras AUC thresholds plus 0.5, the threshold of BinaryAccuracy /
    Precision / Recall (bin = the number of bounds strictly below p).  ``sums`` [T, 4] float64: {n, Σ(p-y)²,
    Σ|p-y|, Σ bce}.  ``update`` is one stream-ordered kernel call (``ot_metrics_update``) with no host sync;
    ``result`` copies the state to the host once and finalises there in float64.  Both tensors are views of
    one buffer, so a reset is one fill and a read one copy.  On a CPU device the object holds, merges and
    finalises state (``load_state`` / ``all_reduce`` / ``result``); ``update`` needs the GPU (no fallback).

    ``weighted=True`` (Keras metrics under ``sample_weight``): the whole state counts in units of 2^-24
    of weight — ``update(..., weights=)`` rounds each weight (clamped to [0, 65536]) to the nearest unit and adds that
    many to its bin, to ``sums[t, 0]`` and, as a factor, to the three sums (``ot_metrics_update_weighted``); a sample
    of zero units is skipped whatever it holds, and an update without weights adds ``WEIGHT_ONE`` = 2^24 units per
    sample.  The integers stay exact and commutative, so the state is as reproducible as the un-weighted one, and
    every reported ratio is the un-weighted formula on it: TP / FP / TN / FN become sums of weights, MSE / MAE /
    logloss Σ w v / Σ w.  (``sums[t, 0]`` is a double holding an integer: exact while a window's weights sum to
    less than 2^29.)
    """

    WEIGHT_ONE = 1 << 24

    def __init__(self, tasks, device, num_thresholds: int = 200, binary_tasks=None, weighted: bool = False):
        import torch
        if binary_tasks is None:
            from .loss import BINARY_TASKS as binary_tasks
        self.tasks = list(tasks)
        self.binary = tuple(t in binary_tasks for t in self.tasks)
        self.device = torch.device(device)
        self.weighted = bool(weighted)
        self.thresholds = keras_thresholds(num_thresholds)
        self.bounds_host = np.unique(np.concatenate([self.thresholds, [0.5]]))        # ascending, 0.5 once
        self.nb = len(self.bounds_host)
        if not 1 <= len(self.tasks) <= 32 or not 1 <= self.nb <= 1024:
            raise ValueError('StreamingMetrics: 1..32 tasks and at most 1024 bounds')
        # threshold j is bounds[at[j]]: #(p > it) = the bins above at[j]
        self.thr_at = np.searchsorted(self.bounds_host, self.thresholds)
        self.half_at = int(np.searchsorted(self.bounds_host, 0.5))
        T, nc = len(self.tasks), len(self.tasks) * 2 * (self.nb + 1)
        self._state = torch.zeros(nc + T * 4, dtype=torch.int64, device=self.device)
        self.counts = self._state[:nc].view(T, 2, self.nb + 1)
        self.sums = self._state[nc:].view(torch.float64).view(T, 4)
        self.bounds = torch.from_numpy(self.bounds_host).to(self.device)

    def update(self, labels, probs, weights=None) -> None:
        """``labels``, ``probs``: [T, B] float32 device tensors (rows contiguous).  No host sync.
        ``weights`` (a ``weighted`` object only): [T, B], or [B] / [1, B] for every task, float32 on the device."""
        import torch
        from . import kernels as K
        if weights is not None and not self.weighted:
            raise ValueError('StreamingMetrics.update: weights need StreamingMetrics(..., weighted=True)')
        if probs.dim() != 2 or probs.shape[0] != len(self.tasks) or labels.shape != probs.shape:
            raise ValueError(f'StreamingMetrics.update: expected two [{len(self.tasks)}, B] tensors')
        if labels.dtype != torch.float32 or probs.dtype != torch.float32:
            raise ValueError('StreamingMetrics.update: float32 tensors expected')
        if probs.device.type != 'cuda' or labels.device != probs.device or self.device.type != 'cuda':
            raise K._lib.OneTransHipError('StreamingMetrics.update runs on the GPU only (there is no CPU fallback)')
        T, B = probs.shape
        if probs.stride(1) != 1 or labels.stride(1) != 1 or (T > 1 and labels.stride(0) != probs.stride(0)):
            labels, probs = labels.contiguous(), probs.contiguous()
        if self.weighted:
            if weights is None:
                weights = torch.ones(B, dtype=torch.float32, device=probs.device)
            if weights.dtype != torch.float32 or weights.device != probs.device:
                raise ValueError('StreamingMetrics.update: weights must be float32 on the device of probs')
            if weights.dim() == 2 and tuple(weights.shape) == (T, B) and T > 1 and weights.stride(0) != 0:
                weights, wstride = weights.contiguous(), B
            elif weights.dim() == 2 and tuple(weights.shape) == (T, B) and T > 1:
                weights, wstride = weights[0].contiguous(), 0                        # one expanded row
            elif weights.numel() == B:
                weights, wstride = weights.reshape(-1).contiguous(), 0
            else:
                raise ValueError(f'StreamingMetrics.update: weights of shape {tuple(weights.shape)}; expected '
                                 f'[{T}, {B}] or [{B}]')
            K.metrics_update_weighted(probs, labels, weights, T, B, probs.stride(0) if T > 1 else B, wstride,
                                      self.bounds, self.nb, self.counts, self.sums, device=probs.device)
            return
        K.metrics_update(probs, labels, T, B, probs.stride(0) if T > 1 else B, self.bounds, self.nb, self.counts,
                         self.sums, device=probs.device)

    def reset_states(self) -> None:
        self._state.zero_()

    def state(self):
        """(counts, sums): the live state tensors."""
        return self.counts, self.sums

    def load_state(self, counts, sums) -> None:
        import torch
        self.counts.copy_(torch.as_tensor(counts).reshape(self.counts.shape))
        self.sums.copy_(torch.as_tensor(sums).reshape(self.sums.shape))

    def all_reduce(self, group=None) -> None:
        """Sum the state over the ranks, in place (what Keras does to metric variables under a distribution
        strategy); a no-op outside an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        dist.all_reduce(self.counts, group=group)
        dist.all_reduce(self.sums, group=group)

    def result(self, extended: bool = False) -> Dict[str, float]:
        """The reference's metric names: ``{t}_auc / _accuracy / _precision / _recall`` for a binary task,
        ``{t}_mse / _mae`` for any other; ``extended`` adds ``{t}_logloss`` and ``{t}_f1`` (evaluate.py:49-50).
        Ratios are Keras's ``div_no_nan``: an empty denominator reports 0."""
        T = len(self.tasks)
        host = self._state.cpu().numpy()                                             # the one D2H copy
        nc = T * 2 * (self.nb + 1)
        counts = host[:nc].reshape(T, 2, self.nb + 1)
        sums = host[nc:].view(np.float64).reshape(T, 4)
        res = {}
        for i, t in enumerate(self.tasks):
            n = sums[i, 0]
            if not self.binary[i]:
                res[f'{t}_mse'] = float(div_no_nan(sums[i, 1], n))
                res[f'{t}_mae'] = float(div_no_nan(sums[i, 2], n))
                continue
            # above[c][j] = #(class c, p > bounds[j]) = the bins j+1.. (suffix sums)
            above = np.cumsum(counts[i, :, ::-1], axis=1)[:, ::-1][:, 1:]
            N, P = (int(v) for v in counts[i].sum(axis=1))
            res[f'{t}_auc'] = roc_trapezoid(above[1][self.thr_at], above[0][self.thr_at], P, N)
            tp, fp = int(above[1][self.half_at]), int(above[0][self.half_at])
            fn, tn = P - tp, N - fp
            prec, rec = float(div_no_nan(tp, tp + fp)), float(div_no_nan(tp, tp + fn))
            res[f'{t}_accuracy'] = float(div_no_nan(tp + tn, P + N))
            res[f'{t}_precision'] = prec
            res[f'{t}_recall'] = rec
            if extended:
                res[f'{t}_f1'] = float(div_no_nan(2.0 * prec * rec, prec + rec))
                res[f'{t}_logloss'] = float(div_no_nan(sums[i, 3], n))
        return res


class GroupedAUC:
    """``uauc`` per binary task as a device-side metric.

    UAUC is not additive: it needs every (group, label, probability) record of the evaluation window, grouped
    and ranked inside each group.  The state is therefore a device log — ids [cap] int64, labels and probs
    [T, cap] float32 — whose fill count is a host integer: ``update`` appends with slice copies (no host sync, no
    kernel of its own) and the log doubles when full.  ``result`` is one ``ot_grouped_auc`` call over the filled
    log and one D2H copy.  ``group_bits``: the caller's promise that every id is below 2^group_bits (for example
    from the vocabulary size); it only shortens the sort.  On a CPU device the object holds and merges state
    (``load_state`` / ``state`` / ``all_gather``, the empty ``result``); ``update`` and a non-empty ``result`` need
    the GPU (no fallback)."""

    def __init__(self, tasks, device, capacity: int = 1 << 20, group_bits: int = 64, binary_tasks=None):
        import torch
        if binary_tasks is None:
            from .loss import BINARY_TASKS as binary_tasks
        self.tasks = list(tasks)
        self.binary = tuple(t in binary_tasks for t in self.tasks)
        self.device = torch.device(device)
        if not 1 <= len(self.tasks) <= 32:
            raise ValueError('GroupedAUC: 1..32 tasks')
        if not 1 <= int(group_bits) <= 64 or int(capacity) < 1:
            raise ValueError('GroupedAUC: group_bits in 1..64 and a positive capacity')
        self.group_bits = int(group_bits)
        self.task_mask = sum(1 << i for i, b in enumerate(self.binary) if b)
        self.count = 0
        self._alloc(int(capacity))

    def _alloc(self, cap: int) -> None:
        import torch
        T = len(self.tasks)
        self.capacity = cap
        self._ids = torch.empty(cap, dtype=torch.int64, device=self.device)
        self._labels = torch.empty(T, cap, dtype=torch.float32, device=self.device)
        self._probs = torch.empty(T, cap, dtype=torch.float32, device=self.device)

    def _reserve(self, total: int) -> None:
        """Room for ``total`` records: the log doubles until they fit, the filled part moves over."""
        if total >= 1 << 31:
            raise ValueError('GroupedAUC: a window holds fewer than 2^31 records')
        if total <= self.capacity:
            return
        cap = self.capacity
        while cap < total:
            cap *= 2
        old, n = (self._ids, self._labels, self._probs), self.count
        self._alloc(cap)
        self._ids[:n].copy_(old[0][:n])
        self._labels[:, :n].copy_(old[1][:, :n])
        self._probs[:, :n].copy_(old[2][:, :n])

    def _append(self, groups, labels, probs) -> None:
        B, n = groups.shape[0], self.count
        self._reserve(n + B)
        self._ids[n:n + B].copy_(groups)
        self._labels[:, n:n + B].copy_(labels)
        self._probs[:, n:n + B].copy_(probs)
        self.count = n + B

    def update(self, groups, labels, probs) -> None:
        """``groups``: [B] or [B, 1] int64; ``labels``, ``probs``: [T, B] float32 (any strides); device tensors.
        No host sync."""
        import torch
        from . import kernels as K
        if probs.dim() != 2 or probs.shape[0] != len(self.tasks) or labels.shape != probs.shape:
            raise ValueError(f'GroupedAUC.update: expected two [{len(self.tasks)}, B] tensors')
        if labels.dtype != torch.float32 or probs.dtype != torch.float32:
            raise ValueError('GroupedAUC.update: float32 tensors expected')
        if groups.dtype != torch.int64 or groups.numel() != probs.shape[1] or groups.dim() > 2:
            raise ValueError('GroupedAUC.update: groups must be B int64 ids ([B] or [B, 1])')
        if (probs.device.type != 'cuda' or labels.device != probs.device or groups.device != probs.device
                or self.device.type != 'cuda'):
            raise K._lib.OneTransHipError('GroupedAUC.update runs on the GPU only (there is no CPU fallback)')
        if probs.shape[1]:
            self._append(groups.reshape(-1), labels, probs)

    def reset_states(self) -> None:
        self.count = 0

    def state(self):
        """(groups [n], labels [T, n], probs [T, n]): views of the filled part of the log."""
        n = self.count
        return self._ids[:n], self._labels[:, :n], self._probs[:, :n]

    def load_state(self, groups, labels, probs) -> None:
        """Replace the log by these records."""
        import torch
        T = len(self.tasks)
        g = torch.as_tensor(groups).reshape(-1).to(torch.int64)
        y = torch.as_tensor(labels).to(torch.float32).reshape(T, -1)
        p = torch.as_tensor(probs).to(torch.float32).reshape(T, -1)
        if not y.shape[1] == p.shape[1] == g.shape[0]:
            raise ValueError('GroupedAUC.load_state: groups [n], labels [T, n] and probs [T, n] expected')
        self.count = 0
        self._append(g, y, p)

    def all_gather(self, group=None) -> None:
        """Every rank's records, on every rank, in rank order.  In a data-parallel run one user's impressions are
        spread over the ranks, so the state cannot be summed: the counts are all-gathered, then the logs, padded to
        the largest count and trimmed.  Every rank then computes the same result.  A no-op outside an initialised
        process group."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        W, T, n = dist.get_world_size(group), len(self.tasks), self.count
        mine = torch.tensor([n], dtype=torch.int64, device=self.device)
        counts = [torch.empty_like(mine) for _ in range(W)]
        dist.all_gather(counts, mine, group=group)
        counts = [int(c) for c in torch.cat(counts).cpu()]
        m = max(counts)
        if m == 0:
            return
        # one int64 and 2T float32 rows per rank, padded to m records
        ids = torch.zeros(m, dtype=torch.int64, device=self.device)
        vals = torch.zeros(2 * T, m, dtype=torch.float32, device=self.device)
        ids[:n].copy_(self._ids[:n])
        vals[:T, :n].copy_(self._labels[:, :n])
        vals[T:, :n].copy_(self._probs[:, :n])
        all_ids = [torch.empty_like(ids) for _ in range(W)]
        all_vals = [torch.empty_like(vals) for _ in range(W)]
        dist.all_gather(all_ids, ids, group=group)
        dist.all_gather(all_vals, vals, group=group)
        self.count = 0
        self._reserve(sum(counts))
        for r, c in enumerate(counts):
            if c:
                self._append(all_ids[r][:c], all_vals[r][:T, :c], all_vals[r][T:, :c])

    def result(self, per_group: bool = False) -> Dict:
        """Per binary task ``{t}_uauc`` (impression-weighted), ``{t}_uauc_macro`` (the plain mean over valid groups),
        ``{t}_uauc_users`` and ``{t}_uauc_impressions`` (the valid groups and their records); ratios are
        ``div_no_nan``.  ``per_group`` adds ``'groups'`` (the distinct ids, ascending as unsigned 64-bit) and
        ``{t}_group_stats`` ([G, 3] int64: n_pos, n_neg, 2U).  An empty log reports zeros without a kernel call."""
        import torch
        from . import kernels as K
        T, n = len(self.tasks), self.count
        agg, G = np.zeros((T, 4)), 0
        ids = stats = None
        if n > 0:
            if self.device.type != 'cuda':
                raise K._lib.OneTransHipError('GroupedAUC.result runs on the GPU only (there is no CPU fallback)')
            out = torch.empty(T * 4 + 1, dtype=torch.int64, device=self.device)
            if per_group:
                ids = torch.empty(n, dtype=torch.int64, device=self.device)
                stats = torch.empty(T, n, 3, dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                K.grouped_auc(self._ids, self._probs, self._labels, T, n, self.capacity, self.group_bits,
                              self.task_mask, out, (out, T * 4), ids, stats, device=self.device)
            host = out.cpu().numpy()                                                 # the one D2H copy
            agg, G = host[:T * 4].view(np.float64).reshape(T, 4), int(host[T * 4])
        res = {}
        if per_group:
            res['groups'] = ids[:G].cpu().numpy() if ids is not None else np.zeros(0, np.int64)
        for i, t in enumerate(self.tasks):
            if not self.binary[i]:
                continue
            res[f'{t}_uauc'] = float(div_no_nan(agg[i, 0], agg[i, 2]))
            res[f'{t}_uauc_macro'] = float(div_no_nan(agg[i, 1], agg[i, 3]))
            res[f'{t}_uauc_users'] = int(agg[i, 3])
            res[f'{t}_uauc_impressions'] = int(agg[i, 2])
            if per_group:
                res[f'{t}_group_stats'] = (stats[i, :G].cpu().numpy() if stats is not None
                                           else np.zeros((0, 3), np.int64))
        return res
