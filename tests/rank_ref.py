"""The yardstick for ot_rank_topk (include/onetrans_hip.h, "ranking"), in plain numpy, written from the
definition: fused scores in float64, the order value of an f32 score with NaN and -0 handled explicitly,
and the per-request top-K as one np.lexsort on (candidate index ascending, order value descending)."""

import numpy as np


def fuse64(probs, weights, mode):
    """probs [T, C] -> float64 [C]: 'sum' = Σ w_t p_t; 'product' = Π p_t over the tasks with w_t != 0."""
    p = np.asarray(probs, np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    if mode == 'sum':
        return (w[:, None] * p).sum(0)
    if mode == 'product':
        f = np.ones(p.shape[1])
        for t in range(p.shape[0]):
            if w[t] != 0:
                f = f * p[t]
        return f
    raise ValueError(mode)


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays, correctly rounded: the product of two f32 values is exact in float64; the
    sum is rounded to odd there (TwoSum's residual tells whether it was inexact and on which side), which makes
    the final rounding to f32 the rounding of the exact value (53 >= 24 + 2 bits)."""
    s = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        t = s + c
        bb = t - s
        e = (s - (t - bb)) + (c - bb)
    odd = (t.view(np.int64) & 1) == 1
    fix = np.isfinite(t) & np.isfinite(e) & (e != 0) & ~odd
    t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(np.float32)


def fuse32(probs, weights, mode):
    """The fused f32 score as the contract defines it: one rounding per task, in task order."""
    p = np.asarray(probs, np.float32)
    w = np.asarray(weights, np.float32)
    if mode == 'sum':
        f = np.zeros(p.shape[1], np.float32)
        for t in range(p.shape[0]):
            f = fma32(np.full_like(f, w[t]), p[t], f)
        return f
    f = np.ones(p.shape[1], np.float32)
    for t in range(p.shape[0]):
        if w[t] != 0:
            f = (f * p[t]).astype(np.float32)
    return f


def orderable(f):
    """f32 [C] -> uint32 with the ranking order: NaN -> 0 (below -inf), -0 -> +0, then the sign flip."""
    f = np.asarray(f, np.float32)
    nan = np.isnan(f)
    g = np.where(nan | (f == 0), np.float32(0.0), f).astype(np.float32)     # -0 -> +0; NaN placeholder
    u = g.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(nan, np.uint32(0), o).astype(np.uint32)


def rank_topk(f, req, R, K):
    """f [C] f32 fused scores, req [C] (outside [0, R): excluded) -> (index [R, K] int32, -1 padded;
    score [R, K] f32, -inf padded; count [R] int32)."""
    f = np.asarray(f, np.float32)
    req = np.asarray(req, np.int64)
    C = f.shape[0]
    idx = np.full((R, K), -1, np.int32)
    score = np.full((R, K), -np.inf, np.float32)
    count = np.zeros(R, np.int32)
    o = orderable(f).astype(np.int64)
    c = np.arange(C, dtype=np.int64)
    for r in range(R):
        mem = c[(req == r)]
        # last key is the primary one: order value descending, then candidate index ascending
        order = mem[np.lexsort((mem, -o[mem]))]
        k = min(K, len(order))
        idx[r, :k] = order[:k]
        score[r, :k] = f[order[:k]]
        count[r] = k
    return idx, score, count


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
