"""ot_rank_topk on the device (kernels.rank_topk, OneTransServer.rank, OneTransInferenceEngine.rank_candidates)
against the numpy yardstick tests/rank_ref.py.  Indices and counts are exact, top_score is bit-equal to
fused_out[top_idx], padding slots are (-1, -inf); the selection is checked on the returned f32 fused scores and
those are pinned by float64 bounds."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd.data import make_batch
from recommend_amd.model import OneTransModel
from recommend_amd.params import init_params
from recommend_amd.serving import OneTransServer

import rank_ref as RR
from test_model_gpu import ns_t, small_criteo

EPS = 2.0 ** -23


def run(dev, probs, req, R, Kk, weights=None, mode='sum', stride_pad=0):
    """probs [T, C] f32 (numpy), req [C] -> (index, score, count, fused) as numpy."""
    probs = np.asarray(probs, np.float32)
    T, C = probs.shape
    weights = [1.0] * T if weights is None else weights
    buf = torch.zeros(T, C + stride_pad, device=dev)
    buf[:, :C] = torch.from_numpy(probs)
    rq = torch.from_numpy(np.asarray(req, np.int32)).to(dev)
    idx = torch.full((R, Kk), 12345, dtype=torch.int32, device=dev)
    sc = torch.full((R, Kk), 7.0, device=dev)
    cnt = torch.full((R,), -5, dtype=torch.int32, device=dev)
    fused = torch.full((C,), 3.0, device=dev)
    K.rank_topk(buf, C + stride_pad, T, weights, mode, rq, C, R, Kk, idx, sc, cnt, fused, device=dev)
    return idx.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy(), fused.cpu().numpy()


def check(dev, probs, req, R, Kk, **kw):
    """The contract: the yardstick's answer on the returned fused scores, bit for bit."""
    idx, sc, cnt, fused = run(dev, probs, req, R, Kk, **kw)
    ridx, rsc, rcnt = RR.rank_topk(fused, req, R, Kk)
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(RR.bits(sc), RR.bits(rsc))
    for r in range(R):
        k = cnt[r]
        np.testing.assert_array_equal(RR.bits(sc[r, :k]), RR.bits(fused[idx[r, :k]]))
        assert (idx[r, k:] == -1).all() and (sc[r, k:] == -np.inf).all()
    return idx, sc, cnt, fused


def test_one_candidate(dev):
    idx, sc, cnt, _ = check(dev, [[0.375]], [0], 1, 1)
    assert idx.tolist() == [[0]] and sc.tolist() == [[0.375]] and cnt.tolist() == [1]


def test_no_candidates(dev):
    idx, sc, cnt, _ = check(dev, np.zeros((2, 0), np.float32), np.zeros(0, np.int32), 3, 4)
    assert (idx == -1).all() and (sc == -np.inf).all() and (cnt == 0).all()


def test_no_requests(dev):
    """R = 0: nothing to write but the fused scores."""
    p = np.array([[0.25, 0.5, 0.75]], np.float32)
    _, _, _, fused = run(dev, p, [0, 0, 0], 0, 2)
    np.testing.assert_array_equal(RR.bits(fused), RR.bits(p[0]))


def test_ragged_requests(dev):
    """Random unsorted req over 5 requests: request 3 is empty and request 1 has fewer than K members."""
    rng = np.random.default_rng(0)
    C = 1000
    req = rng.choice([0, 2, 4], C)
    req[rng.choice(C, 7, replace=False)] = 1
    assert (req == 3).sum() == 0 and (req == 1).sum() == 7
    _, _, cnt, _ = check(dev, rng.random((2, C), np.float32), req, 5, 10, weights=[1.0, 0.5], stride_pad=24)
    assert cnt.tolist() == [10, 7, 10, 0, 10]


@pytest.mark.parametrize('n', [255, 256, 257, 4097])
def test_segment_sizes(dev, n):
    """One request whose size crosses the workgroup width and its stride, next to a small one."""
    rng = np.random.default_rng(n)
    req = np.concatenate([np.zeros(n, np.int32), np.ones(3, np.int32)])
    rng.shuffle(req)
    check(dev, rng.random((1, n + 3), np.float32), req, 2, 17)


@pytest.mark.parametrize('Kk,n', [(1, 300), (64, 300), (100, 300), (1024, 1023), (1024, 1024), (1024, 1025),
                                  (1024, 3000)])
def test_slot_counts(dev, Kk, n):
    rng = np.random.default_rng(Kk + n)
    _, _, cnt, _ = check(dev, rng.standard_normal((1, n)).astype(np.float32), np.zeros(n, np.int32), 1, Kk)
    assert cnt.tolist() == [min(Kk, n)]


def test_all_scores_equal(dev):
    """Every key differs only in its index bits: the select must walk all the way down and still stop at K."""
    n = 700
    req = np.zeros(2 * n, np.int32)
    req[1::2] = 1                                          # request 1 holds the odd candidates
    idx, _, cnt, _ = check(dev, np.full((1, 2 * n), 0.5, np.float32), req, 2, 100)
    assert cnt.tolist() == [100, 100]
    np.testing.assert_array_equal(idx[0], np.arange(0, 200, 2))
    np.testing.assert_array_equal(idx[1], np.arange(1, 200, 2))
    idx, _, _, _ = check(dev, np.full((1, 5000), 0.5, np.float32), np.zeros(5000, np.int32), 1, 100)
    np.testing.assert_array_equal(idx[0], np.arange(100))


@pytest.mark.parametrize('Kk', [1, 37, 100, 1024])
def test_boundary_inside_a_tie_run(dev, Kk):
    rng = np.random.default_rng(3)
    p = rng.choice(np.array([0.125, 0.25, 0.5, 0.75], np.float32), (1, 2500))
    check(dev, p, np.zeros(2500, np.int32), 1, Kk)


def test_special_values(dev):
    rng = np.random.default_rng(4)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 1.0, -1.0, 3e38, -3e38, 0.5],
                    np.float32)
    p = rng.choice(vals, (1, 600))
    req = rng.integers(0, 3, 600)
    for Kk in (5, 300):
        # product mode with one task: f = 1.0f * p keeps the sign of a zero and the denormals
        idx, sc, cnt, fused = check(dev, p, req, 3, Kk, mode='product')
        np.testing.assert_array_equal(RR.bits(fused[~np.isnan(p[0])]), RR.bits(p[0][~np.isnan(p[0])]))
        assert np.isnan(fused[np.isnan(p[0])]).all()
        for r in range(3):
            n_nan = int(np.isnan(p[0][req == r]).sum())
            n_r = int((req == r).sum())
            got_nan = int(np.isnan(sc[r, :cnt[r]]).sum())
            assert got_nan == max(0, min(Kk, n_r) - (n_r - n_nan))      # a NaN only when nothing else is left
    # negative weights turn the order round; sum mode
    check(dev, p, req, 3, 40, weights=[-1.5])
    # every candidate NaN
    idx, sc, cnt, _ = check(dev, np.full((1, 50), np.nan, np.float32), np.zeros(50, np.int32), 1, 8, mode='product')
    assert idx[0].tolist() == list(range(8)) and np.isnan(sc).all()


def test_exclusion(dev):
    rng = np.random.default_rng(5)
    C, R = 900, 4
    req = rng.integers(-1, R + 1, C)                       # -1 and R: excluded
    req[:3] = [-2 ** 31, 2 ** 31 - 1, R]
    p = rng.random((1, C), np.float32)
    members = (req >= 0) & (req < R)
    for Kk in (1024, 10):                                  # every member shown; the select among members only
        idx, _, cnt, _ = check(dev, p, req, R, Kk)
        if Kk == 1024:
            assert cnt.sum() == members.sum()
        shown = idx[idx >= 0]
        assert len(set(shown.tolist())) == len(shown) and members[shown].all()
        for r in range(R):
            assert (req[idx[r, :cnt[r]]] == r).all()


def test_fusion_single_task_is_the_probability(dev):
    p = np.random.default_rng(6).random((1, 777), np.float32)
    _, _, _, fused = check(dev, p, np.zeros(777, np.int32), 1, 5)
    np.testing.assert_array_equal(RR.bits(fused), RR.bits(p[0]))


def test_fusion_weighted_sum(dev):
    p = np.random.default_rng(7).random((3, 777), np.float32)
    w = [0.5, 0.25, 2.0]
    _, _, _, fused = check(dev, p, np.zeros(777, np.int32), 1, 20, weights=w)
    bound = 3 * EPS * (np.abs(np.array(w)[:, None] * p.astype(np.float64))).sum(0)
    err = np.abs(fused.astype(np.float64) - RR.fuse64(p, w, 'sum'))
    assert (err <= bound).all(), (err / bound).max()
    np.testing.assert_array_equal(RR.bits(fused), RR.bits(RR.fuse32(p, w, 'sum')))       # one rounding per fma


def test_fusion_product_drops_zero_weights(dev):
    rng = np.random.default_rng(8)
    p = rng.random((3, 777), np.float32)
    w = [1.0, 0.0, 1.0]
    req = rng.integers(0, 2, 777)
    a = check(dev, p, req, 2, 20, weights=w, mode='product')
    ref = RR.fuse64(p, w, 'product')
    assert (np.abs(a[3].astype(np.float64) - ref) <= 2 * EPS * np.abs(ref)).all()
    p2 = p.copy()
    p2[1] = rng.random(777, np.float32)
    p2[1, :5] = [np.nan, np.inf, 0.0, -1.0, 1e30]
    b = check(dev, p2, req, 2, 20, weights=w, mode='product')
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                      y.view(np.uint32) if y.dtype == np.float32 else y)


def test_order_independence(dev):
    rng = np.random.default_rng(9)
    C, R, Kk = 1500, 4, 33
    p = rng.permutation(C).astype(np.float32)[None] / C     # distinct scores
    req = rng.integers(0, R, C)
    a = check(dev, p, req, R, Kk)
    b = check(dev, p, req, R, Kk)                            # the same call again: the same bits
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    perm = rng.permutation(C)                                # candidate j of the second call is perm[j] of the first
    c = check(dev, p[:, perm], req[perm], R, Kk)
    np.testing.assert_array_equal(c[2], a[2])
    np.testing.assert_array_equal(c[1], a[1])
    np.testing.assert_array_equal(perm[c[0]], a[0])
    # the same membership with req sorted (candidates grouped by request) and shuffled
    order = np.argsort(req, kind='stable')
    d = check(dev, p[:, order], req[order], R, Kk)
    assert (np.diff(req[order]) >= 0).all()
    np.testing.assert_array_equal(d[1], a[1])
    np.testing.assert_array_equal(order[d[0]], a[0])


# ------------------------------------------------------------------ OneTransServer.rank

@pytest.fixture(scope='module')
def served(dev):
    cfg = small_criteo('tail', pyramid=True, layers=3)
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    return cfg, OneTransServer(OneTransModel(cfg, device=dev, init=P))


@pytest.mark.parametrize('Rq,C,k', [(5, 23, 4), (2, 129, 8)])
def test_server_rank(dev, served, Rq, C, k):
    cfg, srv = served
    _, seq_r, _ = make_batch(Rq, cfg, seed=2000)
    ns_c, _, _ = make_batch(C, cfg, seed=3000)
    req = np.random.default_rng(1).integers(0, Rq, C)
    req[:Rq] = np.arange(Rq)
    cache = srv.encode_requests(ns_t(seq_r, dev))
    base = srv.score(cache, torch.from_numpy(req), ns_t(ns_c, dev))
    tasks = list(cfg.tasks)
    wsets = [(None, 'sum'), (None, 'product'),
             ({tasks[0]: 0.25, tasks[-1]: -2.0}, 'sum'), ({tasks[0]: 0.0}, 'product')]
    for weights, mode in wsets:
        out = srv.rank(cache, torch.from_numpy(req), ns_t(ns_c, dev), k, weights=weights, mode=mode,
                       return_probs=True)
        assert out['index'].dtype == torch.int32 and tuple(out['index'].shape) == (Rq, k)
        assert out['score'].dtype == torch.float32 and tuple(out['score'].shape) == (Rq, k)
        assert out['count'].dtype == torch.int32 and tuple(out['count'].shape) == (Rq,)
        for t in tasks:
            assert tuple(out['probs'][t].shape) == (C, 1)
            np.testing.assert_allclose(out['probs'][t].cpu().numpy(), base[t].cpu().numpy(), atol=2e-6, rtol=0)
        p = np.stack([out['probs'][t].cpu().numpy()[:, 0] for t in tasks])
        w = np.array([1.0 if weights is None else weights.get(t, 1.0) for t in tasks], np.float32)
        # the fused f32 score as the contract defines it (one rounding per step), then the yardstick
        ridx, rsc, rcnt = RR.rank_topk(RR.fuse32(p, w, mode), req, Rq, k)
        np.testing.assert_array_equal(out['count'].cpu().numpy(), rcnt)
        np.testing.assert_array_equal(out['index'].cpu().numpy(), ridx)
        np.testing.assert_array_equal(RR.bits(out['score'].cpu().numpy()), RR.bits(rsc))
    assert 'probs' not in srv.rank(cache, torch.from_numpy(req), ns_t(ns_c, dev), k)


def test_server_rank_refuses(dev, served):
    cfg, srv = served
    _, seq_r, _ = make_batch(2, cfg, seed=5)
    ns_c, _, _ = make_batch(4, cfg, seed=6)
    cache = srv.encode_requests(ns_t(seq_r, dev))
    req = torch.tensor([0, 1, 1, 0])
    with pytest.raises(ValueError, match='1..1024'):
        srv.rank(cache, req, ns_t(ns_c, dev), 1025)
    with pytest.raises(ValueError, match='unknown task'):
        srv.rank(cache, req, ns_t(ns_c, dev), 2, weights={'no_such_task': 1.0})
    with pytest.raises(ValueError):
        srv.rank(cache, req, ns_t(ns_c, dev), 2, mode='max')
    with pytest.raises(ValueError):
        srv.rank(cache, torch.tensor([0, 1, 2, 0]), ns_t(ns_c, dev), 2)      # the same validation as score


# ------------------------------------------------------------------ OneTransInferenceEngine.rank_candidates

def test_engine_rank_candidates(dev, tmp_path):
    from recommend_amd.serving import OneTransInferenceEngine
    from recommend_amd.trainer import OneTransTrainer
    cfg = small_criteo('head')
    cfg.max_seq_len = 12
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    tr = OneTransTrainer(cfg, model_dir=str(tmp_path), model=OneTransModel(cfg, device=dev, init=P))
    tr.save_model('m')
    eng = OneTransInferenceEngine(str(tmp_path / 'm'), device=dev)
    ns_c, seq, _ = make_batch(9, cfg, seed=9)
    names = list(ns_c)
    user = {k: ns_c[k][0] for k in names[:5]}
    cands = [{k: ns_c[k][i] for k in names[5:]} for i in range(9)]
    seq1 = {k: v[0] for k, v in seq.items()}
    scored = eng.score_candidates(user, seq1, cands)
    tasks = list(cfg.tasks)
    for mode in ('sum', 'product'):
        before = eng.get_stats()['total_requests']
        got = eng.rank_candidates(user, seq1, cands, 3, mode=mode)
        assert eng.get_stats()['total_requests'] == before + 1 and eng.get_stats()['success_rate'] == 100.0
        assert len(got) == 3
        # score_candidates' output ranked by the same rule
        p = np.array([[s[t] for s in scored] for t in tasks], np.float32)
        ridx, rsc, _ = RR.rank_topk(RR.fuse32(p, [1.0] * len(tasks), mode), np.zeros(9, np.int32), 1, 3)
        assert [g[0] for g in got] == ridx[0].tolist()
        np.testing.assert_array_equal(RR.bits(np.array([g[1] for g in got], np.float32)), RR.bits(rsc[0]))
        for c, _, probs in got:
            assert probs == scored[c]
    assert len(eng.rank_candidates(user, seq1, cands, 20)) == 9              # k beyond the candidates
    with pytest.raises(ValueError):
        eng.rank_candidates(user, seq1, cands, 2000)
    assert eng.get_stats()['failed_requests'] == 1
