"""Float64 numpy reference of the embedding-table update (ot_sparse_adagrad and its two-phase and dense forms) and
the one input the table-kernel tests share.  TEST INFRASTRUCTURE ONLY."""

import functools

import numpy as np

from oracle import keras_math as km

NUM_ROWS = 400
# Step size.  The tests hold the table to rtol 1e-5 / atol 1e-6 (test_sparse_adagrad's tolerances) with the clip off,
# where the update has slope lr / sqrt(0.1) = 3.2 lr in a small row sum g.  The hot key's g is an f32 sum along a
# chain of 68 additions of partial sums of size ~10 (the order the header pins, so its bits are not the kernel's to
# improve): a random walk of 68 roundings of <= 2^-21 / 2 each, ~2.5e-6 rms and ~1e-5 at 4 sigma over a wide row.
# 3.2 lr 1e-5 <= 1e-6 asks for lr <= 0.03.  (At test_sparse_adagrad's own 0.1, whose clip of 3 shrinks g a
# hundredfold, an exact f32 restatement of the update in numpy misses 1e-6 by 16 % at E = 64.)  The smallest wrong
# clip scale these tests are after (0.1 %, E = 12) still moves the hot row by 3.5 times the tolerance at 0.03.
LR, EPS = 0.03, 1e-7
HOT_KEY, HOT_RUN = 7, 200                # one run of four 64-row pieces (64 + 64 + 64 + the rest)
INVALID = (-1, NUM_ROWS, NUM_ROWS + 7, -(1 << 40), 1 << 40)


def unique_row_sums(keys, grads, num_rows):
    """Steps 1-2: drop the keys outside [0, num_rows), sum the gradient rows per key.  -> (unique keys ascending,
    their float64 row sums)."""
    keys = np.asarray(keys)
    ok = (keys >= 0) & (keys < num_rows)
    uk, inv = np.unique(keys[ok], return_inverse=True)
    g = np.zeros((len(uk), grads.shape[1]), np.float64)
    np.add.at(g, inv, np.asarray(grads, np.float64)[ok])
    return uk, g


def sparse_adagrad_ref(table, accum, keys, grads, num_rows, lr, eps, clip):
    """The whole update in float64: de-duplicate, clip_by_norm over the unique rows (clip <= 0: none), Keras Adagrad.
    -> (table, accum, unique keys)."""
    uk, g = unique_row_sums(keys, grads, num_rows)
    if clip > 0:
        g = km.clip_by_norm(g, clip)
    w, a = km.adagrad_sparse_update(np.asarray(table, np.float64), np.asarray(accum, np.float64), uk, g, lr, eps)
    return w, a, uk


@functools.lru_cache(maxsize=None)
def table_inputs(E):
    """~1500 (key, gradient row) pairs on a 400-row table: every row 0..299 at least once (>= 300 unique keys:
    several blocks of the update kernels at every width), one hot key with a run of 200, Zipf-distributed keys for
    the rest, five keys outside the table, all at fixed-seed permuted positions.  Read-only arrays."""
    rng = np.random.default_rng(1100 + E)
    zipf = (rng.zipf(1.2, 995) - 1) % NUM_ROWS
    keys = np.concatenate([np.arange(300), np.full(HOT_RUN, HOT_KEY), zipf, INVALID]).astype(np.int64)
    keys = keys[np.random.default_rng(11).permutation(len(keys))]
    grads = rng.standard_normal((len(keys), E)).astype(np.float32)
    table = rng.uniform(-0.05, 0.05, (NUM_ROWS, E)).astype(np.float32)
    accum = np.full((NUM_ROWS, E), 0.1, np.float32)
    for a in (keys, grads, table, accum):
        a.setflags(write=False)
    return keys, grads, table, accum
