"""Evaluation metrics of the reference trainer/evaluator.

* ``auc`` — exact rank-based ROC AUC (Mann-Whitney U, average ranks for ties): the primary
  parity estimator, identical on both sides.
* ``keras_auc`` — ``tf.keras.metrics.AUC()`` defaults (train.py:101, evaluate.py:45): ROC over 200
  thresholds, trapezoidal interpolation.
Both are host-side numpy over whole arrays of probabilities.
* ``StreamingMetrics`` — the reference's running per-step metrics (AUC, BinaryAccuracy, Precision, Recall; MSE,
  MAE; logloss and F1 for the evaluator) as device state: one HIP launch per step (``ot_metrics_update``), no
  host sync, read once per epoch.
"""

from __future__ import annotations

from typing import Dict

import numpy as np


def auc(labels, scores) -> float:
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
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


def keras_auc(labels, probs, num_thresholds: int = 200) -> float:
    thr = keras_thresholds(num_thresholds)
    y = np.asarray(labels).reshape(-1) > 0.5
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    ps = np.sort(p)
    # counts of predictions > thr via searchsorted (O(n log n))
    gt = len(p) - np.searchsorted(ps, thr, side='right')
    pos_sorted = np.sort(p[y])
    tp = len(pos_sorted) - np.searchsorted(pos_sorted, thr, side='right')
    fp = gt - tp
    return roc_trapezoid(tp, fp, y.sum(), (~y).sum())


class StreamingMetrics:
    """The reference's running Keras metrics (train.py:95-109, evaluate.py:39-56) as additive device state.

    ``counts`` [T, 2, nb+1] int64: per task and label class (``label > 0.5``), a histogram of the probabilities
    over ``bounds`` — the ``num_thresholds`` Keras AUC thresholds plus 0.5, the threshold of BinaryAccuracy /
    Precision / Recall (bin = the number of bounds strictly below p).  ``sums`` [T, 4] float64: {n, Σ(p-y)²,
    Σ|p-y|, Σ bce}.  ``update`` is one stream-ordered kernel call (``ot_metrics_update``) with no host sync;
    ``result`` copies the state to the host once and finalises there in float64.  Both tensors are views of
    one buffer, so a reset is one fill and a read one copy.  On a CPU device the object holds, merges and
    finalises state (``load_state`` / ``all_reduce`` / ``result``); ``update`` needs the GPU (no fallback).
    """

    def __init__(self, tasks, device, num_thresholds: int = 200, binary_tasks=None):
        import torch
        if binary_tasks is None:
            from .model import BINARY_TASKS as binary_tasks
        self.tasks = list(tasks)
        self.binary = tuple(t in binary_tasks for t in self.tasks)
        self.device = torch.device(device)
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

    def update(self, labels, probs) -> None:
        """``labels``, ``probs``: [T, B] float32 device tensors (rows contiguous).  No host sync."""
        import torch
        from . import kernels as K
        if probs.dim() != 2 or probs.shape[0] != len(self.tasks) or labels.shape != probs.shape:
            raise ValueError(f'StreamingMetrics.update: expected two [{len(self.tasks)}, B] tensors')
        if labels.dtype != torch.float32 or probs.dtype != torch.float32:
            raise ValueError('StreamingMetrics.update: float32 tensors expected')
        if probs.device.type != 'cuda' or labels.device != probs.device or self.device.type != 'cuda':
            raise K._lib.OneTransHipError('StreamingMetrics.update runs on the GPU only (there is no CPU fallback)')
        T, B = probs.shape
        if probs.stride(1) != 1 or labels.stride(1) != 1 or (T > 1 and labels.stride(0) != probs.stride(0)):
            labels, probs = labels.contiguous(), probs.contiguous()
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
