"""The embedding-table kernels (embedding.hip, shard.hip) through the C ABI, each against a float64 / exact numpy
restatement: the sparse Adagrad update in its one-call, two-phase (row-sharded) and dense (data-parallel) forms at
every legal kind of row width, and the row-sharding helpers.

Row widths: the update kernels give a segment tps = min(E / 4, 64) threads and a 256-thread block 256 / tps
segments.  WIDTHS holds widths whose tps divides 256 (4, 16, 64, 256, 520, 1024) and widths whose tps does not
(12, 20, 24, 40, 48, 96, 192, 252: the block's last 256 % tps threads belong to no segment of the block)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from oracle import keras_math as km
from table_ref import EPS, HOT_KEY, HOT_RUN, LR, NUM_ROWS, sparse_adagrad_ref, table_inputs, unique_row_sums

WIDTHS = [4, 12, 16, 20, 24, 40, 48, 64, 96, 192, 252, 256, 520, 1024]
MAX_SPB = 85                              # segments per block at E = 12, the most among the widths above


def _bits(x):
    a = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint32)


def _device_inputs(E, dev):
    keys, grads, table, accum = table_inputs(E)
    uk = np.unique(keys[(keys >= 0) & (keys < NUM_ROWS)])
    assert len(uk) >= 3 * MAX_SPB and (keys == HOT_KEY).sum() > HOT_RUN and ((keys < 0) | (keys >= NUM_ROWS)).sum() == 5
    return (keys, grads, table, accum, uk) + tuple(torch.tensor(a, device=dev) for a in (keys, grads, table, accum))


def _check_update(t_d, a_d, w_ref, a_ref, table, accum, uk):
    w, a = t_d.cpu().numpy(), a_d.cpu().numpy()
    rest = np.setdiff1d(np.arange(NUM_ROWS), uk)
    assert len(rest) > 0
    assert np.array_equal(_bits(w[rest]), _bits(table[rest])) and np.array_equal(_bits(a[rest]), _bits(accum[rest]))
    np.testing.assert_allclose(w, w_ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a, a_ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('clip', [0.0, 3.0, 1e6])
@pytest.mark.parametrize('E', WIDTHS)
def test_sparse_adagrad_widths(dev, E, clip):
    """ot_sparse_adagrad vs the float64 reference with the clip off (0), active (3: the gradient norm is
    ~sqrt(1500 E)) and inactive (1e6); rows without a key keep their bits.  With the clip off only the apply kernel
    can move a number: a mismatch there is an update applied twice."""
    keys, grads, table, accum, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    w_ref, a_ref, _ = sparse_adagrad_ref(table, accum, keys, grads, NUM_ROWS, LR, EPS, clip)
    K.sparse_adagrad(t_d, a_d, E, NUM_ROWS, k_d, g_d, len(keys), LR, EPS, clip, device=dev)
    _check_update(t_d, a_d, w_ref, a_ref, table, accum, uk)


@pytest.mark.parametrize('E', WIDTHS)
def test_sparse_prepare_finish_widths(dev, E):
    """The two-phase form as two owners (key % 2) of one table use it: each owner's ot_sparse_prepare squared norm vs
    the float64 norm of its unique-row sums (non-negative addends, a few thousand of them: rtol 1e-5), the norms
    added on the device, each owner's ot_sparse_finish; the table equals the one-call reference with clip 3.  An
    empty owner (n = 0) reports a zero norm and writes nothing else."""
    keys, grads, table, accum, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    clip = 3.0
    owners = []
    total = torch.zeros(1, device=dev)
    for o in range(2):
        sel = np.flatnonzero(keys % 2 == o)
        ko, go = k_d[torch.from_numpy(sel).to(dev)].contiguous(), g_d[torch.from_numpy(sel).to(dev)].contiguous()
        ws = K.sparse_workspace(len(sel), E, dev)
        sumsq = torch.full((1,), -1.0, device=dev)
        K.sparse_prepare(E, NUM_ROWS, ko, go, len(sel), sumsq, ws)
        _, g64 = unique_row_sums(keys[sel], grads[sel], NUM_ROWS)
        np.testing.assert_allclose(float(sumsq.item()), float((g64 * g64).sum()), rtol=1e-5)
        total += sumsq
        owners.append((len(sel), ws, ko, go))
    for n_o, ws, _, _ in owners:
        K.sparse_finish(t_d, a_d, E, n_o, LR, EPS, clip, total, ws)
    w_ref, a_ref, _ = sparse_adagrad_ref(table, accum, keys, grads, NUM_ROWS, LR, EPS, clip)
    _check_update(t_d, a_d, w_ref, a_ref, table, accum, uk)

    before_t, before_a = _bits(t_d), _bits(a_d)
    ws = torch.full((256,), 0xAB, dtype=torch.uint8, device=dev)
    sumsq = torch.full((4,), 5.0, device=dev)
    K.sparse_prepare(E, NUM_ROWS, k_d, g_d, 0, sumsq, ws)
    assert sumsq.cpu().tolist() == [0.0, 5.0, 5.0, 5.0]
    K.sparse_finish(t_d, a_d, E, 0, LR, EPS, clip, total, ws)
    assert bool((ws == 0xAB).all())
    assert np.array_equal(_bits(t_d), before_t) and np.array_equal(_bits(a_d), before_a)


@pytest.mark.parametrize('E', WIDTHS)
def test_dense_form_matches_sparse_widths(dev, E):
    """ot_sparse_grad_dense + ot_dense_adagrad equal ot_sparse_adagrad (test_dense_exchange_matches_sparse's
    tolerances, clip 3: active).  The dense buffer itself vs the float64 per-key sums: a key's m rows are added in
    f32 along a chain of at most min(m, 64) + ceil(m / 64) additions (pieces of 64, then the pieces), so the error
    is at most that many times 2^-24 of the key's sum of |g| (the standard bound for a sequential sum)."""
    keys, grads, table, accum, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    n, clip = len(keys), 3.0
    t1, a1 = t_d.clone(), a_d.clone()
    K.sparse_adagrad(t1, a1, E, NUM_ROWS, k_d, g_d, n, LR, EPS, clip, device=dev)
    dense = torch.zeros(NUM_ROWS, E, device=dev)
    K.sparse_grad_dense(E, NUM_ROWS, k_d, g_d, n, dense, device=dev)
    t2, a2 = t_d.clone(), a_d.clone()
    K.dense_adagrad(t2, a2, dense, NUM_ROWS, E, LR, EPS, clip, device=dev)
    torch.testing.assert_close(t2, t1, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(a2, a1, rtol=1e-5, atol=1e-6)

    _, g64 = unique_row_sums(keys, grads, NUM_ROWS)
    _, mag = unique_row_sums(keys, np.abs(grads), NUM_ROWS)
    m = np.array([(keys == k).sum() for k in uk])
    chain = np.minimum(m, 64) + (m + 63) // 64
    d = dense.cpu().numpy()
    assert (np.abs(d[uk] - g64) <= (chain * 2.0 ** -24)[:, None] * mag).all()
    rest = np.setdiff1d(np.arange(NUM_ROWS), uk)
    assert not _bits(d[rest]).any()
    assert np.array_equal(_bits(t2)[rest], _bits(table)[rest]) and np.array_equal(_bits(a2)[rest], _bits(accum)[rest])


@pytest.mark.parametrize('n', [0, 1, 1000])
@pytest.mark.parametrize('E', [4, 24, 64, 520])
def test_gather_permute_rows(dev, E, n):
    """ot_gather_rows (negative index: a zero row) and ot_permute_rows (there with inverse = 0, back with
    inverse = 1) move bits: both equal numpy indexing exactly; n = 0 writes nothing."""
    rng = np.random.default_rng(100 * E + n)
    R = 50
    table = rng.standard_normal((R, E)).astype(np.float32)
    idx = rng.integers(-3, R, max(n, 1)).astype(np.int64)
    if n > 2:
        idx[:3] = [-1, R - 1, 0]
    out = torch.full((max(n, 1), E), 7.0, device=dev)
    K.gather_rows(torch.from_numpy(table).to(dev), E, torch.from_numpy(idx).to(dev), n, out)
    exp = np.full((max(n, 1), E), 7.0, np.float32)
    exp[:n] = np.where(idx[:n, None] >= 0, table[np.maximum(idx[:n], 0)], np.float32(0))
    assert np.array_equal(_bits(out), _bits(exp))

    src = rng.standard_normal((max(n, 1), E)).astype(np.float32)
    perm = rng.permutation(max(n, 1)).astype(np.int32)
    s_d, p_d = torch.from_numpy(src).to(dev), torch.from_numpy(perm).to(dev)
    there = torch.full((max(n, 1), E), 7.0, device=dev)
    back = torch.full((max(n, 1), E), 7.0, device=dev)
    K.permute_rows(s_d, p_d, n, E, 0, there)
    K.permute_rows(there, p_d, n, E, 1, back)
    exp = np.full((max(n, 1), E), 7.0, np.float32)
    exp[:n] = src[perm[:n]]
    assert np.array_equal(_bits(there), _bits(exp))
    exp[:n] = src[:n]
    assert np.array_equal(_bits(back), _bits(exp))


@pytest.mark.parametrize('n', [0, 1, 5000])
@pytest.mark.parametrize('world', [1, 3, 8])
def test_shard_route_kernel(dev, world, n):
    """ot_shard_route vs the header's contract: owner = id % world (an id outside [0, num_rows): owner 0), perm =
    the positions ordered by owner, stable; send_local[j] = id / world of the j-th routed id (-1 outside);
    counts[r] = ids routed to rank r."""
    num_rows = 100_003
    rng = np.random.default_rng(7 * n + world)
    ids = ((rng.zipf(1.2, n) - 1) % num_rows).astype(np.int64)
    if n > 5:
        ids[[0, 17, 400, n - 1]] = [-5, num_rows, num_rows + 7, -1]
        ids[1] = num_rows - 1
    perm = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    send_local = torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev)
    counts = torch.full((world + 1,), -7, dtype=torch.int32, device=dev)
    K.shard_route(torch.from_numpy(ids).to(dev) if n else torch.zeros(1, dtype=torch.int64, device=dev), n, num_rows,
                  world, perm, send_local, counts)
    ok = (ids >= 0) & (ids < num_rows)
    owner = np.where(ok, ids % world, 0)
    local = np.where(ok, ids // world, -1)
    order = np.argsort(owner, kind='stable')
    assert counts.cpu().tolist() == np.bincount(owner, minlength=world).tolist() + [-7]
    if n == 0:
        assert perm.cpu().tolist() == [-7] and send_local.cpu().tolist() == [-7]
        return
    assert np.array_equal(perm.cpu().numpy(), order)
    assert np.array_equal(send_local.cpu().numpy(), local[order])


def _hash_uniform_ref(rows, E, seed, lo, hi):
    """hash_uniform_rows_kernel restated: two fmix32 rounds over the element's global index, the top 24 bits as
    u in [0, 1), lo + (hi - lo) u with one rounding (the product and the sum are exact in float64 here)."""
    gid = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(E, dtype=np.uint64)[None, :]
    idx = ((gid * np.uint64(E) + c) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    h1 = km.fmix32(idx * np.uint32(0x9E3779B1) + np.uint32(seed))
    h2 = km.fmix32(h1 ^ (gid >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x85EBCA77))
    u = (h2 >> np.uint32(8)).astype(np.float64) / 16777216.0
    span = np.float32(hi) - np.float32(lo)
    return (np.float64(span) * u + np.float64(np.float32(lo))).astype(np.float32)


@pytest.mark.parametrize('E', [4, 17, 64])
def test_hash_uniform_rows(dev, E):
    """ot_hash_uniform_rows: the logical table (global row = local row * world + rank) is the same bits whatever the
    world size, equals the numpy restatement, and lies in [lo, hi)."""
    rows, seed, lo, hi = 1000, 0xC0FFEE11, -0.05, 0.05
    ref = _hash_uniform_ref(rows, E, seed, lo, hi)
    assert (ref >= np.float32(lo)).all() and (ref < np.float32(hi)).all() and len(np.unique(ref)) > rows * E * 0.99
    for world in [1, 2, 3, 8]:
        logical = np.full((rows, E), np.nan, np.float32)
        for rank in range(world):
            local_rows = len(range(rank, rows, world))
            out = torch.full((local_rows + 1, E), 9.0, device=dev)
            K.hash_uniform_rows(out, local_rows, E, rank, world, seed, lo, hi)
            out = out.cpu().numpy()
            assert (out[local_rows] == 9.0).all()
            logical[rank::world] = out[:local_rows]
        assert np.array_equal(_bits(logical), _bits(ref)), world
