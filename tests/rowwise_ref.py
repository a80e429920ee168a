"""Float64 numpy reference of the row-wise Adagrad table update (ot_sparse_adagrad_rowwise and its two-phase and
dense forms), and an f32 restatement of the same arithmetic.  TEST INFRASTRUCTURE ONLY.

The rule, for a table W [rows, E] and an accumulator A [rows]: de-duplicate and clip exactly as the element-wise
update does (table_ref.unique_row_sums, keras_math.clip_by_norm), then for every unique valid key r with clipped
row g:  A[r] += (sum_c g[c]^2) / E ;  W[r, c] -= lr g[c] / sqrt(A[r] + eps)."""

import numpy as np

from oracle import keras_math as km
from table_ref import unique_row_sums

# The GPU tests' tolerances: the element-wise table tests' own (test_table_kernels_gpu._check_update).  Their
# derivation in table_ref.py carries over: W still has slope at most lr / sqrt(0.1) in a row sum g, and the
# accumulator's own error (a mean of E squares, each good to ~1e-7 relative) moves W by about 2e-8 at the hot key.
W_TOL = dict(rtol=1e-5, atol=1e-6)
A_TOL = dict(rtol=1e-5, atol=1e-5)


def rowwise_adagrad_ref(table, accum_rows, keys, grads, num_rows, lr, eps, clip):
    """The whole update in float64.  -> (table, accum_rows, unique keys)."""
    uk, g = unique_row_sums(keys, grads, num_rows)
    if clip > 0:
        g = km.clip_by_norm(g, clip)
    return rowwise_apply_ref(table, accum_rows, uk, g, lr, eps) + (uk,)


def rowwise_apply_ref(table, accum_rows, uk, g, lr, eps):
    """The rule on unique rows ``uk`` with (clipped) float64 row gradients ``g``.  -> (table, accum_rows)."""
    w, a = np.array(table, np.float64), np.array(accum_rows, np.float64)
    a[uk] += (g * g).sum(1) / g.shape[1]
    w[uk] -= lr * g / np.sqrt(a[uk] + eps)[:, None]
    return w, a


def rowwise_adagrad_f32(table, accum_rows, keys, grads, num_rows, lr, eps, clip):
    """The same update with every operation rounded to float32 and every sum taken sequentially: per key the rows in
    position order, the squared norm over the unique rows in order, a row's sum of squares column by column.  No
    kernel is asked to add in this order; it shows that f32 arithmetic of this kind meets W_TOL / A_TOL."""
    f = np.float32
    keys = np.asarray(keys)
    ok = np.flatnonzero((keys >= 0) & (keys < num_rows))
    uk = np.unique(keys[ok])
    slot = {int(k): i for i, k in enumerate(uk)}
    g = np.zeros((len(uk), grads.shape[1]), f)
    for i in ok:                                         # position order within every key
        g[slot[int(keys[i])]] += grads[i]
    if clip > 0:
        sq = f(0)
        for row in g:
            sq = f(sq + np.cumsum(row * row, dtype=f)[-1])
        g = g * (f(clip) / max(np.sqrt(sq, dtype=f), f(clip)))
    E = g.shape[1]
    w, a = np.array(table, f), np.array(accum_rows, f)
    ssq = np.cumsum(g * g, axis=1, dtype=f)[:, -1]       # sequential f32 adds
    a[uk] = a[uk] + ssq / f(E)
    den = np.sqrt(a[uk] + f(eps), dtype=f)
    w[uk] = w[uk] - (f(lr) * g) / den[:, None]
    assert w.dtype == f and a.dtype == f and g.dtype == f
    return w, a, uk
