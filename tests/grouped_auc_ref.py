"""The yardstick of the grouped-AUC tests: the impression-weighted user-level AUC written from its definition, with a
Python loop over the groups and explicit pair counting (O(n_pos * n_neg) per group).  Independent of
``recommend_amd.metrics``.

For one binary task over records (g_i, y_i, s_i):
  * the class is y_i > 0.5;
  * the score order is the order of the f32 values; -0.0 ties with +0.0; every NaN ties with every other NaN and
    ranks above +inf (arbitrary but fixed);
  * per distinct group u: n_pos, n_neg and 2U = sum over (pos p, neg q) in u of (2 [s_p > s_q] + [s_p == s_q]);
  * a group is valid with n_pos > 0 and n_neg > 0; then AUC_u = 2U / (2 n_pos n_neg);
  * UAUC = sum_valid n_u AUC_u / sum_valid n_u, n_u = n_pos + n_neg; 0 with no valid group.
The distinct groups are listed in ascending order of their ids read as unsigned 64-bit integers.
"""

import functools

import numpy as np

SPECIAL = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, np.inf, np.nan], dtype=np.float32)


def rank_value(scores):
    """f32 scores -> float64 values with the order of the definition: finite values as they are (-0.0 == +0.0 in
    float arithmetic), -inf / +inf beyond every finite f32, NaN above +inf."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    v = np.where(np.isnan(s), np.inf, s)
    v = np.where(np.isposinf(s), 1e300, v)
    v = np.where(np.isneginf(s), -1e300, v)
    return v


def ref_uauc(groups, labels, scores):
    """{'ids': [G] int64, 'stats': [G, 3] int64 (n_pos, n_neg, 2U), 'agg': [4] float64 (sum n_u AUC_u, sum AUC_u,
    sum n_u, #valid), 'uauc', 'uauc_macro', 'users', 'impressions'} of one task."""
    g = np.asarray(groups, dtype=np.int64).reshape(-1)
    pos = np.asarray(labels).reshape(-1) > 0.5
    v = rank_value(np.asarray(scores).reshape(-1))
    ids = sorted({int(x) for x in g}, key=lambda x: x & (2 ** 64 - 1))
    stats = []
    agg = [0.0, 0.0, 0.0, 0.0]
    for u in ids:
        m = g == u
        vp, vn = v[m & pos], v[m & ~pos]
        gt = int(np.count_nonzero(vp[:, None] > vn[None, :]))
        eq = int(np.count_nonzero(vp[:, None] == vn[None, :]))
        npos, nneg, u2 = len(vp), len(vn), 2 * gt + eq
        stats.append((npos, nneg, u2))
        if npos > 0 and nneg > 0:
            a = float(u2) / (2.0 * npos * nneg)
            agg[0] += (npos + nneg) * a
            agg[1] += a
            agg[2] += npos + nneg
            agg[3] += 1.0
    return {'ids': np.array(ids, dtype=np.int64), 'stats': np.array(stats, dtype=np.int64).reshape(-1, 3),
            'agg': np.array(agg), 'uauc': agg[0] / agg[2] if agg[2] > 0 else 0.0,
            'uauc_macro': agg[1] / agg[3] if agg[3] > 0 else 0.0, 'users': int(agg[3]), 'impressions': int(agg[2])}


def rel_close(a, b, rtol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b))))


def zipf_groups(rng, n, card):
    return ((rng.zipf(1.3, size=n) - 1) % card).astype(np.int64)


# name -> (T, n, group_bits, binary mask over the tasks)
CASES = {
    'one_record': (1, 1, 64, (True,)),
    'one_group': (1, 63, 64, (True,)),
    'all_distinct': (2, 65, 64, (True, True)),
    'ties': (2, 257, 64, (True, True)),
    'zipf_crawler': (2, 4096, 64, (True, True)),
    'wide_ids_masked': (3, 10007, 64, (True, True, False)),
    'zipf_crawler_min_bits': (2, 4096, None, (True, True)),     # group_bits: the minimum that fits the ids
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(groups [n] int64, labels [T, n] f32, scores [T, n] f32, group_bits, binary, [per-task ref_uauc or None]):
    computed once, shared, read-only."""
    T, n, bits, binary = CASES[name]
    rng = np.random.default_rng(1000 * T + n)
    y = (rng.random((T, n)) < 0.4).astype(np.float32)
    # probabilities on a coarse grid as well, so that ties happen among ordinary values too
    s = np.where(rng.random((T, n)) < 0.5, rng.random((T, n)), rng.integers(0, 8, (T, n)) / 8.0).astype(np.float32)
    if name == 'one_record':
        g = np.array([5], dtype=np.int64)
    elif name == 'one_group':
        g = np.full(n, 3, dtype=np.int64)
    elif name == 'all_distinct':
        g = rng.permutation(n).astype(np.int64) * 7
    elif name == 'ties':
        g = rng.integers(0, 7, n).astype(np.int64)
        s = SPECIAL[rng.integers(0, len(SPECIAL), (T, n))]
    elif name.startswith('zipf_crawler'):
        g = zipf_groups(rng, n, 500)
        g[rng.permutation(n)[:2000]] = 499                # the crawler: one group of (at least) 2000 records
    else:
        g = zipf_groups(rng, n, 3000) * 1000003 + (1 << 40)
        g[::97] = -1 - (g[::97] % 5)                      # top bit set: the largest ids as unsigned 64-bit
        y[2] = rng.random(n).astype(np.float32)           # a regression task: not binary, masked off
    if bits is None:
        bits = max(1, int(g.max()).bit_length())
    refs = [ref_uauc(g, y[t], s[t]) if binary[t] else None for t in range(T)]
    for a in (g, y, s):
        a.setflags(write=False)
    return g, y, s, bits, binary, refs
