"""Timestamp-aware sequence fusion on the GPU (``seq_fusion='time'``): ot_seq_time_rows against the host order
(tests/time_fusion_ref.py), the tokenizer bit for bit against the concatenation it permutes, the model against the
float64 oracle with the time-fused tokenizer, mode isolation, input errors and the serving path."""

import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import _lib
from recommend_amd import kernels as K
from recommend_amd.data import make_batch
from recommend_amd.layout import TILE, build_map, round_up
from recommend_amd.model import OneTransModel, _Tokenize
from recommend_amd.params import init_params, keras_variables
from recommend_amd.serving import OneTransServer
from recommend_amd.trainer import OneTransTrainer
from oracle import onetrans_ref as R

import time_fusion_ref as TF
from test_model_gpu import LOGIT_TOL, c1, check_grads, ns_t, setup, small_criteo

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
GUARD = 256


# ------------------------------------------------------------------ the kernel
def run_kernel(dev, times, groups=None, ngroups=None, row_stride=None, ws_bytes=None):
    """ot_seq_time_rows on ``times`` (one [B, L_i] int64 array per present sequence) whose sequences are the weight
    groups ``groups`` of an ``ngroups``-group row map built as the model builds it (layout.build_map: every group
    padded to whole tiles with -1).  Returns (map buffer, rank, last_time) with guard bands behind each, and
    the map's (offset, B * L) segments."""
    B = times[0].shape[0]
    lens = [t.shape[1] for t in times]
    L_S = sum(lens)
    groups = list(range(len(times))) if groups is None else groups
    ngroups = ngroups or (max(groups) + 1)
    per_group = [[np.zeros(0, np.int64)] for _ in range(ngroups)]
    for g, L in zip(groups, lens):
        per_group[g] = [np.full(B * L, -5, np.int64)]                    # a real entry the kernel must overwrite
    rm = build_map(per_group)
    starts = np.concatenate([[0], np.cumsum([round_up(len(pg[0]), TILE) for pg in per_group])])
    offs = [int(starts[g]) for g in groups]
    rows = torch.from_numpy(np.concatenate([rm.rows[0], np.full(GUARD, -7, np.int32)])).to(dev)
    rank = torch.full((B * L_S + GUARD,), -7, dtype=torch.int32, device=dev)
    last = torch.full((B + GUARD,), -7, dtype=torch.int64, device=dev)
    tdev = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in times]
    descs = K.seq_time_descs([(t, L, L, off) for t, L, off in zip(tdev, lens, offs)])
    stride = L_S + 3 if row_stride is None else row_stride
    err = None
    try:
        if ws_bytes is None:
            K.seq_time_rows(descs, len(times), B, L_S, stride, rows, rank_out=rank, last_time=last, device=dev)
        else:
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            _lib.call('ot_seq_time_rows', ctypes.cast(descs, ctypes.c_void_p), len(times), B, L_S, stride,
                      rows.data_ptr(), rank.data_ptr(), last.data_ptr(), ws.data_ptr(), ws_bytes,
                      torch.cuda.current_stream().cuda_stream)
    except _lib.OneTransHipError as e:          # a refused call: the caller looks at what it left behind
        err = e
    torch.cuda.synchronize()
    segs = [(o, B * L) for o, L in zip(offs, lens)]
    return rows.cpu().numpy(), rank.cpu().numpy(), last.cpu().numpy(), segs, stride, err


def assert_untouched(rows, rank, last):
    """Buffers as run_kernel made them: real map entries -5, map padding -1, everything else the guard value."""
    assert np.isin(rows[:-GUARD], (-5, -1)).all() and (rows[-GUARD:] == -7).all()
    assert (rank == -7).all() and (last == -7).all()


def check_kernel(dev, times, **kw):
    times = [np.asarray(t, dtype=np.int64) for t in times]
    rows, rank, last, segs, stride, err = run_kernel(dev, times, **kw)
    assert err is None, err
    B = times[0].shape[0]
    L_S = sum(t.shape[1] for t in times)
    want = TF.merge_ranks(times)                                         # [B, L_S], concatenation order
    got = rank[:B * L_S].reshape(B, L_S)
    assert np.array_equal(got, want)
    assert (np.sort(got, axis=1) == np.arange(L_S)).all()                # a permutation per sample
    touched = np.zeros(len(rows), bool)
    c0 = 0
    for (off, n), t in zip(segs, times):
        L = t.shape[1]
        exp = np.arange(B)[:, None] * stride + want[:, c0:c0 + L]
        assert np.array_equal(rows[off:off + n].reshape(B, L), exp)
        touched[off:off + n] = True
        c0 += L
    body = ~touched
    body[-GUARD:] = False
    assert (rows[body] == -1).all()                                      # the map's padding
    assert (rows[-GUARD:] == -7).all() and (rank[B * L_S:] == -7).all() and (last[B:] == -7).all()
    assert np.array_equal(last[:B], np.concatenate(times, axis=1).max(axis=1))


def rand_times(rng, B, lens, lo=0, hi=12):
    return [rng.integers(lo, hi, size=(B, L)) for L in lens]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('lens', [(5, 1, 7), (64, 63, 1)])
def test_kernel_small_ragged(dev, B, lens):
    check_kernel(dev, rand_times(np.random.default_rng(B + lens[0]), B, lens))       # many ties


def test_kernel_absent_sequence(dev):
    """Two of three configured sequences present: their segments sit at the offsets of the three-group map."""
    t = rand_times(np.random.default_rng(2), 3, (5, 7))
    check_kernel(dev, t, groups=[0, 2], ngroups=3)
    check_kernel(dev, t, groups=[1, 2], ngroups=3)


def test_kernel_all_tied(dev):
    check_kernel(dev, [np.full((3, 5), 42), np.full((3, 1), 42), np.full((3, 7), 42)])


def test_kernel_descending_sequence(dev):
    rng = np.random.default_rng(4)
    t = [np.sort(x, axis=1) for x in rand_times(rng, 3, (64, 63, 1), hi=200)]
    t[1] = np.sort(rng.permutation(500)[:63 * 3].reshape(3, 63), axis=1)[:, ::-1].copy()   # strictly descending
    check_kernel(dev, t)


def test_kernel_random_unsorted(dev):
    rng = np.random.default_rng(5)
    check_kernel(dev, [rng.integers(I64_MIN, I64_MAX, size=(3, L), endpoint=True) for L in (64, 63, 1)])
    check_kernel(dev, [rng.integers(I64_MIN, I64_MAX, size=(129, L), endpoint=True) for L in (5, 1, 7)])


def test_kernel_extreme_values(dev):
    vals = np.array([I64_MIN, -1, 0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, I64_MAX, I64_MIN, I64_MAX, -2 ** 32, 1, -1, 0],
                    dtype=np.int64)
    rng = np.random.default_rng(6)
    check_kernel(dev, [rng.choice(vals, size=(3, L)) for L in (5, 1, 7)])
    check_kernel(dev, [rng.permutation(vals)[None, :], rng.permutation(vals)[None, :]])
    check_kernel(dev, [np.full((2, 3), I64_MAX), np.full((2, 2), I64_MAX)])  # real events equal to the sort's padding


def test_kernel_maximum_length(dev):
    rng = np.random.default_rng(7)
    check_kernel(dev, rand_times(rng, 2, (2000, 2095, 1), hi=3000))
    check_kernel(dev, rand_times(rng, 2, (1, 2047, 1), hi=50))           # one short of a power of two


def test_kernel_over_the_limit_writes_nothing(dev):
    t = rand_times(np.random.default_rng(8), 2, (2000, 2096, 1))
    rows, rank, last, _, _, err = run_kernel(dev, t)
    assert err is not None and 'L_S=4097 unsupported' in str(err)
    assert_untouched(rows, rank, last)


def test_kernel_empty_batch(dev):
    rows, rank, last, _, _, err = run_kernel(dev, [np.zeros((0, 5), np.int64), np.zeros((0, 7), np.int64)])
    assert err is None
    assert (rows == -7).all() and (rank == -7).all() and (last == -7).all()


def test_kernel_short_workspace(dev):
    t = rand_times(np.random.default_rng(9), 3, (5, 1, 7))
    need = _lib.size('ot_seq_time_rows_workspace_size', 3, 3, 13)
    assert need > 0
    rows, rank, last, _, _, err = run_kernel(dev, t, ws_bytes=need - 1)
    assert err is not None and 'workspace too small' in str(err)
    assert_untouched(rows, rank, last)
    rows, rank, last, _, _, err = run_kernel(dev, t, ws_bytes=need)
    assert err is None and np.array_equal(rank[:39].reshape(3, 13), TF.merge_ranks(t))


# ------------------------------------------------------------------ the tokenizer, bit for bit
def time_cfg(cfg):
    cfg.seq_fusion = 'time'
    return cfg


def concat_times(B, lens):
    """Times under which the time order is the plain concatenation."""
    out, c = [], 0
    for L in lens:
        out.append(np.tile(np.arange(c, c + L, dtype=np.int64), (B, 1)))
        c += L
    return out


def test_tokenizer_is_the_permuted_concatenation(dev):
    cfg = time_cfg(small_criteo(seq_lens=(5, 9, 7)))
    B, d, L_S = 37, cfg.hidden_dim, 21
    L0 = L_S + cfg.num_ns_tokens
    P, model, (ns, seq, _) = setup(cfg, B, dev)
    names = cfg.feature_config['sequence_features']
    arb = [seq[n + '_time'] for n in names]
    rank = TF.merge_ranks(arb)
    assert (rank != np.arange(L_S)).any()
    # token row of every concatenation-order row under the arbitrary times (NS rows stay)
    perm = np.concatenate([rank, np.tile(np.arange(L_S, L0), (B, 1))], axis=1)
    perm = torch.from_numpy((np.arange(B)[:, None] * L0 + perm).reshape(-1)).to(dev)
    dx_cat = torch.randn(B * L0, d, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    dx_arb = torch.empty_like(dx_cat)
    dx_arb[perm] = dx_cat
    res = []
    for times, dx in ((concat_times(B, (5, 9, 7)), dx_cat), (arb, dx_arb)):
        s = dict(seq)
        s.update({n + '_time': t for n, t in zip(names, times)})
        model.flat.grad.fill_(float('nan'))
        with K.precision(model.matmul):
            plan = model._plan(ns_t(ns, dev), ns_t(s, dev))
            assert plan['L_S'] == L_S and plan['n_sep'] == 0
            x0 = _Tokenize.apply(model.flat, model, plan)
        x0.backward(dx)
        torch.cuda.synchronize()
        (tname, keys, demb), = [p for p in model._pending_sparse if p[0] == 'emb.seq_item']
        res.append((x0.detach().clone(), model.g('tok.seq.kernel').clone(), model.g('tok.seq.bias').clone(),
                    keys.clone(), demb.clone(), model.g('tok.sep').clone(), model.g('tok.ns.kernel').clone()))
    cat, arb_ = res
    assert torch.isfinite(cat[0]).all()
    assert torch.equal(arb_[0][perm], cat[0])                            # x0, row by row
    for i in (1, 2, 3, 4, 6):
        assert torch.equal(arb_[i], cat[i]), i
    assert cat[1].abs().max() > 0 and cat[4].abs().max() > 0
    assert (cat[5] == 0).all() and (arb_[5] == 0).all()                  # [SEP] is unused


# ------------------------------------------------------------------ the model against the float64 oracle
MODEL_CASES = {
    'head': lambda: small_criteo('head'),
    'tail_pyramid': lambda: small_criteo('tail', pyramid=True, layers=3),
    'd128_pyramid': lambda: small_criteo('tail', pyramid=True, layers=3, d=128, H=4, f=256, Lns=12,
                                         seq_lens=(20, 20, 20)),
}


@pytest.fixture
def time_oracle(monkeypatch):
    monkeypatch.setattr(R, 'tokenizer', TF.tokenizer_time)


@pytest.mark.parametrize('case', list(MODEL_CASES))
def test_forward_parity(dev, time_oracle, case):
    cfg = time_cfg(MODEL_CASES[case]())
    P, model, (ns, seq, _) = setup(cfg, 37, dev)
    with torch.no_grad():
        out = model((ns_t(ns, dev), ns_t(seq, dev)), training=False)
    ref = R.forward(R.to_torch(P), cfg, R.to_torch(ns), R.to_torch(seq), training=False)
    assert ref['logits'][cfg.tasks[0]].shape[0] == 37
    for t in cfg.tasks:
        lg = model._last_logits[cfg.tasks.index(t)].double().cpu().numpy()
        np.testing.assert_allclose(lg, ref['logits'][t].numpy()[:, 0], atol=LOGIT_TOL, rtol=0)
        np.testing.assert_allclose(out[t].double().cpu().numpy(), ref['probs'][t].numpy(), atol=LOGIT_TOL / 4, rtol=0)
    # the order matters to the model: the same events in concatenation order score differently
    s = dict(seq)
    names = cfg.feature_config['sequence_features']
    s.update({n + '_time': t for n, t in zip(names, concat_times(37, [seq[n].shape[1] for n in names]))})
    with torch.no_grad():
        other = model((ns_t(ns, dev), ns_t(s, dev)), training=False)
    assert (other[cfg.tasks[0]] - out[cfg.tasks[0]]).abs().max().item() > 1e-6


@pytest.mark.parametrize('case', list(MODEL_CASES))
@pytest.mark.parametrize('training', [False, True])
def test_gradient_parity(dev, time_oracle, case, training):
    check_grads(time_cfg(MODEL_CASES[case]()), 37, dev, training)


def test_gradient_parity_float_event_features(dev, time_oracle):
    """The reference's input form (C1: [B, L, 64] float events, no item table): the same map drives the staged
    event rows."""
    cfg = time_cfg(c1('head'))
    check_grads(cfg, 64, dev, True)
    _, seq, _ = make_batch(4, cfg, seed=1)
    assert seq['click_seq'].dtype == np.float32 and seq['click_seq_time'].shape == seq['click_seq'].shape[:2]


@pytest.mark.parametrize('case', list(MODEL_CASES))
def test_train_steps_parity(dev, time_oracle, case):
    """Three optimizer steps against the oracle (test_model_gpu.test_train_steps_parity's method and bounds); the
    unused [SEP] parameter has an exactly zero gradient and keeps its value."""
    cfg = time_cfg(MODEL_CASES[case]())
    cfg.optimizer_config = dict(cfg.optimizer_config, dense_lr=0.001, momentum=0.9)
    B = 37
    P, model, _ = setup(cfg, B, dev)
    tr = OneTransTrainer(cfg, model=model)
    Pt = R.to_torch(P)
    st = R.init_state(Pt, cfg)
    kv = keras_variables(cfg, {k: v.shape for k, v in P.items() if not k.startswith('emb.')})
    sep0 = model.p('tok.sep').clone()
    for step in range(3):
        batch = make_batch(B, cfg, seed=2000 + step)
        out = tr.train_step(batch)
        assert (model.g('tok.sep') == 0).all()
        seed = (model.dropout_seed + 0x9E3779B9 * model._step) & 0xFFFFFFFF
        ns, seq, lab = batch
        Pt, st, rl, _ = R.train_step(Pt, st, cfg, kv, R.to_torch(ns), R.to_torch(seq), R.to_torch(lab), seed=seed)
        assert abs(out['total_loss'].item() - rl.item()) < 2e-4, step
    got = model.param_dict()
    for name, ref in Pt.items():
        err = np.abs(got[name] - ref.detach().numpy()).max()
        assert err < 2e-4, f'{name} after 3 steps: {err:.2e}'
    assert torch.equal(model.p('tok.sep'), sep0)


def test_second_forward_before_backward_is_refused(dev):
    """The per-call row map and times are staged in place: the generation guard covers them."""
    cfg = time_cfg(small_criteo('head'))
    P, model, (ns, seq, lab) = setup(cfg, 5, dev)
    assert model.time_fusion
    probs = model.forward_probs(ns_t(ns, dev), ns_t(seq, dev), training=False)
    model.forward_probs(ns_t(ns, dev), ns_t(seq, dev), training=False)
    with pytest.raises(RuntimeError, match='second forward'):
        probs.sum().backward()


def test_layers_above_the_model_take_the_times(dev, tmp_path):
    """val_step, the prefetcher, progressive_validation, fit and the offline evaluator with ``*_time`` entries: the
    same batch gives the same loss by every route, and the loops run."""
    from recommend_amd.evaluate import OneTransEvaluator
    from recommend_amd.features import DevicePrefetcher
    cfg = time_cfg(small_criteo('head'))
    P, model, _ = setup(cfg, 16, dev)
    tr = OneTransTrainer(cfg, model_dir=str(tmp_path), model=model)
    batches = [make_batch(16, cfg, seed=300 + i) for i in range(2)]
    direct = [tr.val_step(b)['total_loss'].item() for b in batches]
    pre = list(DevicePrefetcher(batches, dev))
    assert pre[0][1]['click_seq_time'].dtype == torch.int64 and pre[0][1]['click_seq_time'].is_cuda
    assert [tr.val_step(b)['total_loss'].item() for b in pre] == direct
    res = OneTransEvaluator(model, cfg).evaluate_offline(batches)
    assert res['performance']['total_samples'] == 32 and np.isfinite(res['ctr_logloss'])
    pv = tr.progressive_validation(batches)
    assert list(pv['periods']) == [0] and 0.0 <= pv['macro']['ctr_accuracy'] <= 1.0
    hist = tr.fit(batches, batches[:1], epochs=1, save_freq=10)
    assert np.isfinite(hist['train_loss'][0]) and np.isfinite(hist['val_loss'][0])


# ------------------------------------------------------------------ mode isolation and input errors
def test_sep_model_ignores_times(dev):
    cfg = small_criteo('head')
    P, model, (ns, seq, _) = setup(cfg, 37, dev)
    tcfg = time_cfg(copy.deepcopy(cfg))
    _, seq_t, _ = make_batch(37, tcfg, seed=1000)
    assert set(seq_t) > set(seq)
    with torch.no_grad():
        model((ns_t(ns, dev), ns_t(seq, dev)), training=False)
        a = model._last_logits.clone()
        model((ns_t(ns, dev), ns_t(seq_t, dev)), training=False)
        b = model._last_logits.clone()
    assert torch.equal(a, b)


def test_input_errors(dev):
    cfg = time_cfg(small_criteo('head'))
    P, model, (ns, seq, _) = setup(cfg, 6, dev)
    nsd = ns_t(ns, dev)
    fwd = lambda s: model((nsd, ns_t(s, dev)), training=False)
    s = {k: v for k, v in seq.items() if k != 'cart_seq_time'}
    with pytest.raises(ValueError, match="'cart_seq'"):
        fwd(s)
    s = dict(seq, purchase_seq_time=seq['purchase_seq_time'][:, :-1])
    with pytest.raises(ValueError, match="'purchase_seq'.*shape"):
        fwd(s)
    s = dict(seq, click_seq_time=seq['click_seq_time'].astype(np.float64))
    with pytest.raises(TypeError, match="'click_seq'"):
        fwd(s)
    s = dict(seq, click_seq_time=seq['click_seq_time'].astype(np.int32))            # widened
    with torch.no_grad():
        a = fwd(s)[cfg.tasks[0]]
        b = fwd(seq)[cfg.tasks[0]]
    assert torch.equal(a, b)
    bad = copy.deepcopy(cfg)
    bad.seq_fusion = 'nearest'
    with pytest.raises(ValueError, match='seq_fusion'):
        OneTransModel(bad, device=dev)


def test_sharded_table_is_refused(dev):
    cfg = time_cfg(small_criteo('head'))
    cfg.table_sharding = 'row'
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    assert 'emb.seq_item' in model.sharded
    ns, seq, _ = make_batch(6, cfg, seed=1000)
    with pytest.raises(NotImplementedError, match='row-sharded'):
        model((ns_t(ns, dev), ns_t(seq, dev)), training=False)


# ------------------------------------------------------------------ serving
def expand(seq, req):
    return {k: v[req] for k, v in seq.items()}


@pytest.mark.parametrize('case', ['head', 'tail_pyramid'])
def test_cached_serving_matches_forward(dev, time_oracle, case):
    """encode_requests + score equals the full forward on the expanded batch and the oracle (test_serving_gpu's
    method and bounds)."""
    cfg = time_cfg(MODEL_CASES[case]())
    Rq, C = 5, 23
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    _, seq_r, _ = make_batch(Rq, cfg, seed=2000)
    ns_c, _, _ = make_batch(C, cfg, seed=3000)
    req = np.random.default_rng(1).integers(0, Rq, C)
    req[:Rq] = np.arange(Rq)
    srv = OneTransServer(model)
    cache = srv.encode_requests(ns_t(seq_r, dev))
    names = cfg.feature_config['sequence_features']
    want_last = np.concatenate([seq_r[n + '_time'] for n in names], axis=1).max(axis=1)
    assert np.array_equal(cache.last_time.cpu().numpy(), want_last)
    got = srv.score(cache, torch.from_numpy(req), ns_t(ns_c, dev))
    seq_full = expand(seq_r, req)
    with torch.no_grad():
        full = model((ns_t(ns_c, dev), ns_t(seq_full, dev)), training=False)
    ref = R.forward(R.to_torch(P), cfg, R.to_torch(ns_c), R.to_torch(seq_full), training=False)
    for t in cfg.tasks:
        a = got[t].double().cpu().numpy()
        np.testing.assert_allclose(a, full[t].double().cpu().numpy(), atol=2e-6, rtol=0)
        np.testing.assert_allclose(a, ref['probs'][t].numpy(), atol=5e-5, rtol=0)


def _extend_setup(dev, dedicated='head'):
    cfg = time_cfg(small_criteo(dedicated))
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    _, seq_r, _ = make_batch(3, cfg, seed=41)
    ns_c, _, _ = make_batch(9, cfg, seed=42)
    names = cfg.feature_config['sequence_features']
    last = np.concatenate([seq_r[n + '_time'] for n in names], axis=1).max(axis=1)
    return cfg, model, OneTransServer(model), seq_r, ns_c, names, last


@pytest.mark.parametrize('which', [0, 1, 2])
def test_extend_requests_any_sequence(dev, which):
    """New events of the FIRST (or any) configured sequence, later than everything cached, extend the cache to what
    a full re-encode gives; the new events arrive unsorted and tied among themselves."""
    cfg, model, srv, seq_r, ns_c, names, last = _extend_setup(dev, 'head' if which != 1 else 'tail')
    name, dL = names[which], 4
    rng = np.random.default_rng(5)
    new = rng.integers(0, cfg.seq_item_vocab, (3, dL))
    new_t = last[:, None] + np.array([[3, 1, 3, 2]])                      # later; out of order, one tie
    full = dict(seq_r)
    full[name] = np.concatenate([seq_r[name], new], 1)
    full[name + '_time'] = np.concatenate([seq_r[name + '_time'], new_t], 1)
    req = torch.tensor([0, 1, 2, 2, 1, 0, 0, 1, 2])
    ext = srv.extend_requests(srv.encode_requests(ns_t(seq_r, dev)), name, torch.from_numpy(new).to(dev),
                              torch.from_numpy(new_t).to(dev))
    ref_cache = srv.encode_requests(ns_t(full, dev))
    assert ext.L_S == ref_cache.L_S
    assert torch.equal(ext.last_time, ref_cache.last_time)
    a = srv.score(ext, req, ns_t(ns_c, dev))
    b = srv.score(ref_cache, req, ns_t(ns_c, dev))
    with torch.no_grad():
        f = model((ns_t(ns_c, dev), ns_t(expand(full, req.numpy()), dev)), training=False)
    for t in cfg.tasks:
        np.testing.assert_allclose(a[t].cpu().numpy(), b[t].cpu().numpy(), atol=2e-6, rtol=0)
        np.testing.assert_allclose(a[t].cpu().numpy(), f[t].cpu().numpy(), atol=2e-6, rtol=0)
    # a second extension, of another sequence, on top of the first (host times this time)
    name2 = names[(which + 1) % 3]
    new_t2 = new_t.max(axis=1)[:, None] + np.array([[1, 2]])
    new2 = rng.integers(0, cfg.seq_item_vocab, (3, 2))
    ext2 = srv.extend_requests(ext, name2, torch.from_numpy(new2).to(dev), new_t2)
    full[name2] = np.concatenate([full[name2], new2], 1)
    full[name2 + '_time'] = np.concatenate([full[name2 + '_time'], new_t2], 1)
    a = srv.score(ext2, req, ns_t(ns_c, dev))
    b = srv.score(srv.encode_requests(ns_t(full, dev)), req, ns_t(ns_c, dev))
    for t in cfg.tasks:
        np.testing.assert_allclose(a[t].cpu().numpy(), b[t].cpu().numpy(), atol=2e-6, rtol=0)


def test_extend_requests_refuses_events_that_would_not_land_last(dev):
    cfg, model, srv, seq_r, ns_c, names, last = _extend_setup(dev)
    cache = srv.encode_requests(ns_t(seq_r, dev))
    new = torch.zeros(3, 2, dtype=torch.int64, device=dev)
    later = last[:, None] + np.array([[1, 2]])
    early = later.copy()
    early[1, 1] = last[1] - 1                                            # one request, one event too early
    tie = later.copy()
    tie[2, 0] = last[2]
    for name in names:
        with pytest.raises(ValueError, match='earlier than|not later than'):
            srv.extend_requests(cache, name, new, torch.from_numpy(early).to(dev))
    for name in names[:-1]:                                              # a tie is certain to sort last only there
        with pytest.raises(ValueError, match='not later than'):
            srv.extend_requests(cache, name, new, torch.from_numpy(tie))
    ext = srv.extend_requests(cache, names[-1], new, torch.from_numpy(tie))
    full = dict(seq_r)
    full[names[-1]] = np.concatenate([seq_r[names[-1]], new.cpu().numpy()], 1)
    full[names[-1] + '_time'] = np.concatenate([seq_r[names[-1] + '_time'], tie], 1)
    req = torch.arange(9) % 3
    a = srv.score(ext, req, ns_t(ns_c, dev))
    b = srv.score(srv.encode_requests(ns_t(full, dev)), req, ns_t(ns_c, dev))
    for t in cfg.tasks:
        np.testing.assert_allclose(a[t].cpu().numpy(), b[t].cpu().numpy(), atol=2e-6, rtol=0)
    with pytest.raises(ValueError, match='new_times'):
        srv.extend_requests(cache, names[0], new)
    with pytest.raises(TypeError):
        srv.extend_requests(cache, names[0], new, torch.from_numpy(later.astype(np.float32)))
    with pytest.raises(ValueError, match='shape'):
        srv.extend_requests(cache, names[0], new, torch.from_numpy(later[:, :1]))
    with pytest.raises(ValueError, match='not a configured sequence'):
        srv.extend_requests(cache, 'view_seq', new, torch.from_numpy(later))


def test_inference_engine_forwards_times(dev, tmp_path):
    """The engine surface in 'time' mode: times are left-padded with INT64_MIN, and single / batch inference and the
    two-stage score_candidates agree."""
    from recommend_amd.serving import OneTransInferenceEngine
    cfg = time_cfg(small_criteo('head'))
    cfg.max_seq_len = 12
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    tr = OneTransTrainer(cfg, model_dir=str(tmp_path), model=OneTransModel(cfg, device=dev, init=P))
    tr.save_model('m')
    eng = OneTransInferenceEngine(str(tmp_path / 'm'), device=dev)
    assert eng.config.seq_fusion == 'time'
    ns_c, seq, _ = make_batch(4, cfg, seed=9)
    names = list(ns_c)
    user = {k: ns_c[k][0] for k in names[:5]}
    cands = [{k: ns_c[k][i] for k in names[5:]} for i in range(4)]
    seq1 = {k: v[0] for k, v in seq.items()}                      # one user's sequences and times (unpadded)
    _, pre = eng.preprocess_input({}, {}, {}, seq1)
    assert pre['click_seq_time'].dtype == np.int64 and pre['click_seq_time'][0] == I64_MIN
    assert pre['click_seq_time'].shape == (12,) and pre['click_seq'].shape == (12,)
    got = eng.batch_inference([(user, c, {}, seq1) for c in cands])
    single = eng.single_inference(user, cands[2], {}, seq1)
    fast = eng.score_candidates(user, seq1, cands)
    top = eng.rank_candidates(user, seq1, cands, 2)
    for t in cfg.tasks:
        assert abs(single[t] - got[2][t]) < 2e-6
        for i in range(4):
            assert abs(fast[i][t] - got[i][t]) < 2e-6
    assert len(top) == 2 and abs(top[0][2][cfg.tasks[0]] - got[top[0][0]][cfg.tasks[0]]) < 2e-6
