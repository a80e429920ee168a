"""The group-wise NS tokenizer on the GPU (``ns_tokenizer = 'group'``): ot_ns_group_fwd / _bwd_input / _bwd_weight
against float64 numpy within the forward-error bound of an f32 dot product, and the model, trainer, serving,
request-grouped, recompute and checkpoint paths against the oracle whose tokenizer is patched to the grouped one
(tests/ns_groups_ref.py)."""

import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ns_groups_ref as NG
import test_model_gpu as TM
from test_model_gpu import LOGIT_TOL, check_grads, ns_t, setup, small_criteo
from recommend_amd import kernels as K
from recommend_amd.config import ns_group_layout
from recommend_amd.data import expand_requests, make_batch
from recommend_amd.model import OneTransModel, _Tokenize, keras_bce_loss
from recommend_amd.params import init_params, keras_variables
from recommend_amd.serving import OneTransServer
from recommend_amd.trainer import OneTransTrainer, stack_labels
from oracle import onetrans_ref as R

SENTINEL = np.float32(-12345.678)
U = 2.0 ** -24                                     # unit roundoff of f32
WIDTHS = (1, 3, 16, 35, 67)                        # K_g = 1, a width past a 32-k stage with a ragged tail, G = 5
WIDTHS12 = (2, 1, 40, 5, 9, 64, 33, 4, 1, 17, 65, 8)


# =============================================================================== kernels
@functools.lru_cache(maxsize=None)
def kernel_case(B, d, widths):
    """Host data and float64 results of one call of each kernel, built once.  Strides are not the used widths."""
    G = len(widths)
    goff = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)
    ktot = int(goff[-1])
    rng = np.random.default_rng(100 * B + d + G)
    lda, ldx = ktot + 3, G * d + 8
    A = rng.normal(size=(B, lda)).astype(np.float32)
    W = rng.normal(size=(ktot, d)).astype(np.float32)
    bias = rng.normal(size=(G, d)).astype(np.float32)
    D = rng.normal(size=(B, ldx)).astype(np.float32)
    A64, W64, D64 = A.astype(np.float64), W.astype(np.float64), D.astype(np.float64)
    ref = dict(X=np.zeros((B, G, d)), Xb=np.zeros((B, G, d)), dA=np.zeros((B, ktot)), dAb=np.zeros((B, ktot)),
               dW=np.zeros((ktot, d)), dWb=np.zeros((ktot, d)), db=np.zeros((G, d)), dbb=np.zeros((G, d)))
    for g in range(G):
        k0, k1 = goff[g], goff[g + 1]
        a, w, dd = A64[:, k0:k1], W64[k0:k1], D64[:, g * d:(g + 1) * d]
        ref['X'][:, g] = a @ w + bias[g]
        ref['Xb'][:, g] = (k1 - k0 + 2) * U * (np.abs(a) @ np.abs(w) + np.abs(bias[g]))
        ref['dA'][:, k0:k1] = dd @ w.T
        ref['dAb'][:, k0:k1] = (d + 2) * U * (np.abs(dd) @ np.abs(w).T)
        ref['dW'][k0:k1] = a.T @ dd
        ref['dWb'][k0:k1] = (B + 2) * U * (np.abs(a).T @ np.abs(dd))
        ref['db'][g] = dd.sum(axis=0)
        ref['dbb'][g] = (B + 2) * U * np.abs(dd).sum(axis=0)
    return dict(G=G, goff=goff, ktot=ktot, kmax=int(max(widths)), lda=lda, ldx=ldx, A=A, W=W, bias=bias, D=D, **ref)


def fenced(n, dev, pad=4):
    """A sentinel-filled buffer with ``pad`` floats in front of and behind the n the kernel may write."""
    buf = torch.full((n + 2 * pad,), float(SENTINEL), device=dev)
    return buf, (buf, pad)


def untouched(a):
    return np.all(a.view(np.int32) == SENTINEL.view(np.int32))


CASES = [(B, d, WIDTHS) for B in (1, 37, 130) for d in (64, 128, 384)] + [(37, 128, WIDTHS12)]


@pytest.mark.parametrize('B,d,widths', CASES)
def test_kernels_against_float64(dev, B, d, widths):
    c = kernel_case(B, d, widths)
    G, ktot, kmax, lda, ldx = c['G'], c['ktot'], c['kmax'], c['lda'], c['ldx']
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ('goff', 'A', 'W', 'bias', 'D')}
    # ---- forward: token g at columns g*d of a row of stride ldx > G*d; everything around it stays as it was
    xbuf, X = fenced(B * ldx, dev)
    K.ns_group_fwd(t['A'], lda, t['goff'], G, ktot, kmax, t['W'], t['bias'], B, d, X, ldx)
    x = xbuf.cpu().numpy()
    assert untouched(x[:4]) and untouched(x[-4:])
    x = x[4:-4].reshape(B, ldx)
    assert untouched(x[:, G * d:])
    err = np.abs(x[:, :G * d].astype(np.float64).reshape(B, G, d) - c['X'])
    print(f'fwd: max err / bound {float((err / c["Xb"]).max()):.3f}')
    assert np.all(err <= c['Xb'])
    # ---- input gradient: every column of every group's range, nothing past goff[G]
    abuf, dA = fenced(B * lda, dev)
    K.ns_group_bwd_input(t['D'], ldx, t['goff'], G, ktot, kmax, t['W'], B, d, dA, lda)
    a = abuf.cpu().numpy()
    assert untouched(a[:4]) and untouched(a[-4:])
    a = a[4:-4].reshape(B, lda)
    assert untouched(a[:, ktot:])
    err = np.abs(a[:, :ktot].astype(np.float64) - c['dA'])
    print(f'bwd_input: max err / bound {float((err / c["dAb"]).max()):.3f}')
    assert np.all(err <= c['dAb'])
    # ---- weight gradient: two runs bit-identical; accumulate adds exactly onto what dW / db hold
    runs = []
    for _ in range(2):
        wbuf, dW = fenced(ktot * d, dev)
        bbuf, db = fenced(G * d, dev)
        K.ns_group_bwd_weight(t['A'], lda, t['D'], ldx, t['goff'], G, ktot, kmax, B, d, dW, db, device=dev)
        runs.append((wbuf.cpu().numpy(), bbuf.cpu().numpy()))
    assert np.array_equal(runs[0][0].view(np.int32), runs[1][0].view(np.int32))
    assert np.array_equal(runs[0][1].view(np.int32), runs[1][1].view(np.int32))
    w, b = runs[0]
    assert untouched(w[:4]) and untouched(w[-4:]) and untouched(b[:4]) and untouched(b[-4:])
    w, b = w[4:-4].reshape(ktot, d), b[4:-4].reshape(G, d)
    errw, errb = np.abs(w.astype(np.float64) - c['dW']), np.abs(b.astype(np.float64) - c['db'])
    print(f'bwd_weight: dW max err / bound {float((errw / c["dWb"]).max()):.3f}, '
          f'db {float((errb / c["dbb"]).max()):.3f}')
    assert np.all(errw <= c['dWb']) and np.all(errb <= c['dbb'])
    rng = np.random.default_rng(7)
    w0, b0 = rng.normal(size=(ktot, d)).astype(np.float32), rng.normal(size=(G, d)).astype(np.float32)
    dW, db = torch.from_numpy(w0).to(dev), torch.from_numpy(b0).to(dev)
    K.ns_group_bwd_weight(t['A'], lda, t['D'], ldx, t['goff'], G, ktot, kmax, B, d, dW, db, accumulate=True, device=dev)
    assert np.array_equal(dW.cpu().numpy().view(np.int32), (w0 + w).view(np.int32))
    assert np.array_equal(db.cpu().numpy().view(np.int32), (b0 + b).view(np.int32))


# =============================================================================== model
def grouped(cfg):
    return NG.with_groups(cfg)


CONFIGS = {
    'd64_L4': lambda: grouped(small_criteo('head')),
    'd128_L12_pyramid': lambda: grouped(small_criteo('tail', pyramid=True, layers=3, d=128, H=4, f=256, Lns=12,
                                                     seq_lens=(20, 20, 20))),
}


def assert_outputs(model, out, ref, cfg):
    for t in cfg.tasks:
        lg = model._last_logits[cfg.tasks.index(t)].double().cpu().numpy()
        np.testing.assert_allclose(lg, ref['logits'][t].numpy()[:, 0], atol=LOGIT_TOL, rtol=0)
        np.testing.assert_allclose(out[t].double().cpu().numpy(), ref['probs'][t].numpy(), atol=LOGIT_TOL / 4, rtol=0)


@pytest.mark.parametrize('case', list(CONFIGS))
def test_forward_parity(dev, monkeypatch, case):
    cfg = CONFIGS[case]()
    lay = ns_group_layout(cfg)
    order = [cfg.ns_feature_names().index(n) for m in lay['members'] for n in m]
    assert lay['widths'][0] == 1 and order != sorted(order)              # a K_g = 1 group; non-contiguous groups
    assert all({cfg.ns_feature_width(n) for n in m} == {1, cfg.ns_embedding_dim} for m in lay['members'][1:3])
    P, model, batch = setup(cfg, 37, dev)
    ns, seq, _ = batch
    with torch.no_grad():
        out = model((ns_t(ns, dev), ns_t(seq, dev)), training=False)
    # the untouched oracle on the block-structured auto-split parameters
    cfg_a, Pa = NG.expand_to_auto(cfg, P)
    assert_outputs(model, out, TM.oracle_out(Pa, cfg_a, batch), cfg)
    # the oracle with the grouped tokenizer
    monkeypatch.setattr(R, 'tokenizer', NG.tokenizer_groups)
    ref = TM.oracle_out(P, cfg, batch)
    assert_outputs(model, out, ref, cfg)
    # a batch without one group's features (its token is the group's bias) and without a few others
    gone = set(lay['members'][1]) | {lay['members'][2][0], lay['members'][0][0]}
    ns1 = {k: v for k, v in ns.items() if k not in gone}
    with torch.no_grad():
        out1 = model((ns_t(ns1, dev), ns_t(seq, dev)), training=False)
    ref1 = TM.oracle_out(P, cfg, (ns1, seq, None))
    assert_outputs(model, out1, ref1, cfg)
    assert np.abs(ref1['logits'][cfg.tasks[0]].numpy() - ref['logits'][cfg.tasks[0]].numpy()).max() > 10 * LOGIT_TOL


@pytest.mark.parametrize('training', [False, True])
def test_gradient_parity(dev, monkeypatch, training):
    monkeypatch.setattr(R, 'tokenizer', NG.tokenizer_groups)
    check_grads(CONFIGS['d64_L4'](), 37, dev, training)


def test_gradient_parity_d128_pyramid(dev, monkeypatch):
    monkeypatch.setattr(R, 'tokenizer', NG.tokenizer_groups)
    check_grads(CONFIGS['d128_L12_pyramid'](), 37, dev, True)


def test_three_train_steps(dev, monkeypatch):
    """Loss and every parameter after three steps against the oracle's train_step, whose clip units are the per-group
    kernels and biases (keras_variables)."""
    monkeypatch.setattr(R, 'tokenizer', NG.tokenizer_groups)
    cfg = CONFIGS['d64_L4']()
    cfg.optimizer_config = dict(cfg.optimizer_config, dense_lr=0.001, momentum=0.9)
    cfg.gradient_clip_norm = 0.05                  # small enough that the per-group units really clip
    B = 37
    P, model, _ = setup(cfg, B, dev)
    tr = OneTransTrainer(cfg, model=model)
    Pt = R.to_torch(P)
    st = R.init_state(Pt, cfg)
    kv = keras_variables(cfg, {k: v.shape for k, v in P.items() if not k.startswith('emb.')})
    assert len([v for v in kv if v[0] == 'tok.ns.kernel']) == cfg.num_ns_tokens
    for step in range(3):
        batch = make_batch(B, cfg, seed=2000 + step)
        ns, seq, lab = batch
        out = tr.train_step(batch)
        seed = (model.dropout_seed + 0x9E3779B9 * model._step) & 0xFFFFFFFF
        Pt, st, rl, _ = R.train_step(Pt, st, cfg, kv, R.to_torch(ns), R.to_torch(seq), R.to_torch(lab), seed=seed)
        print(f'step {step}: loss {out["total_loss"].item():.6f} vs {rl.item():.6f}')
        assert abs(out['total_loss'].item() - rl.item()) < 2e-4, step
    got = model.param_dict()
    for name, ref in Pt.items():
        err = np.abs(got[name] - ref.detach().numpy()).max()
        assert err < 2e-4, f'{name} after 3 steps: {err:.2e}'
    assert np.abs(got['tok.ns.kernel'] - P['tok.ns.kernel']).max() > 1e-4
    assert got['tok.ns.kernel'].shape == P['tok.ns.kernel'].shape and got['tok.ns.bias'].shape == P['tok.ns.bias'].shape


def test_with_bags(dev, monkeypatch):
    """bag_criteo plus groups: the pooled bags enter their groups' column ranges; forward and every gradient."""
    from test_ns_bags_gpu import _BagModel, bag_criteo, with_out_of_range
    monkeypatch.setattr(R, 'tokenizer', NG.tokenizer_groups)
    monkeypatch.setattr(TM, 'OneTransModel', _BagModel)
    cfg = grouped(bag_criteo())
    lay = ns_group_layout(cfg)
    assert all(any(n in m for m in lay['members'][1:]) for n in cfg.bag_features)
    real_setup = TM.setup
    seen = {}

    def setup_seen(cfg_, B, dev_, seed=0):
        P, model, batch = real_setup(cfg_, B, dev_, seed)
        seen.update(P=P, model=model, batch=with_out_of_range(batch, cfg_))
        return P, model, seen['batch']

    monkeypatch.setattr(TM, 'setup', setup_seen)
    check_grads(cfg, 37, dev, True)
    model, (ns, seq, _) = seen['model'], seen['batch']
    with torch.no_grad():
        out = model((ns_t(ns, dev), ns_t(seq, dev)), training=False)
    assert_outputs(model, out, TM.oracle_out(seen['P'], cfg, seen['batch']), cfg)


def test_a_groups_features_move_only_its_token(dev):
    cfg = CONFIGS['d64_L4']()
    P, model, batch = setup(cfg, 37, dev)
    ns, seq, _ = batch
    L, d = cfg.num_ns_tokens, cfg.hidden_dim

    def tokens(ns_):
        with torch.no_grad(), K.precision(model.matmul):
            plan = model._plan(ns_t(ns_, dev), ns_t(seq, dev))
            return _Tokenize.apply(model.flat, model, plan).view(37, plan['L0'], d).cpu().numpy()

    base = tokens(ns)
    for g, members in enumerate(ns_group_layout(cfg)['members']):
        zeroed = dict(ns)
        for n in members:
            zeroed[n] = np.zeros_like(ns[n])                # dense value 0 / id 0
        got = tokens(zeroed)
        same = np.ones(base.shape[1], bool)
        same[base.shape[1] - L + g] = False
        assert np.array_equal(got[:, same].view(np.int32), base[:, same].view(np.int32)), g
        assert np.abs(got[:, ~same] - base[:, ~same]).max() > 1e-3, g


def test_serving_scores_equal_the_full_forward(dev):
    cfg = grouped(small_criteo('tail', pyramid=True, layers=3))
    Rq, C = 5, 23
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    _, seq_r, _ = make_batch(Rq, cfg, seed=2000)
    ns_c, _, _ = make_batch(C, cfg, seed=3000)
    req = np.random.default_rng(1).integers(0, Rq, C)
    req[:Rq] = np.arange(Rq)
    srv = OneTransServer(model)
    cache = srv.encode_requests(ns_t(seq_r, dev))
    got = srv.score(cache, torch.from_numpy(req), ns_t(ns_c, dev))
    seq_full = {k: v[req] for k, v in seq_r.items()}
    with torch.no_grad():
        full = model((ns_t(ns_c, dev), ns_t(seq_full, dev)), training=False)
    for t in cfg.tasks:
        np.testing.assert_allclose(got[t].double().cpu().numpy(), full[t].double().cpu().numpy(), atol=2e-6, rtol=0)
    top = srv.rank(cache, torch.from_numpy(np.sort(req)), ns_t(ns_c, dev), 3)
    assert tuple(top['index'].shape) == (Rq, 3)


def test_request_grouped_training_equals_the_expanded_batch(dev, monkeypatch):
    import test_request_train_gpu as RT
    monkeypatch.setattr(R, 'tokenizer', NG.tokenizer_groups)
    cfg = grouped(RT.small())
    P, model, batch = RT.case(cfg, dev)
    got = RT.run_requests(model, cfg, batch, dev, training=False)
    RT.compare(got, RT.run_expanded(model, cfg, batch, dev), 2, 'vs expanded')
    RT.compare(got, RT.oracle_side(P, cfg, batch), 1, 'vs oracle', oracle_b=True)
    ns, seq, _, req = batch
    out = model.forward_requests(ns_t(ns, dev), ns_t(seq, dev), torch.from_numpy(req).to(dev))
    ns_e, seq_e, _ = expand_requests(batch)
    with torch.no_grad():
        full = model((ns_t(ns_e, dev), ns_t(seq_e, dev)), training=False)
    for t in cfg.tasks:
        assert (out[t].detach() - full[t]).abs().max().item() < 2 * RT.PROB_TOL


def test_recompute_is_bit_identical_to_the_saved_path(dev):
    cfg = CONFIGS['d128_L12_pyramid']()
    cfg.dropout_rate = 0.1
    P, model, batch = setup(cfg, 41, dev)
    ns, seq, lab = batch
    y = stack_labels(lab, cfg.tasks, dev)
    res = []
    for rc in (False, True):
        model.recompute = rc
        model.flat.grad.zero_()
        model._step = 0
        loss = keras_bce_loss(y, model.forward_probs(ns_t(ns, dev), ns_t(seq, dev), training=True))
        loss.backward()
        sparse = [(k, keys.clone(), g.clone()) for (k, keys, g) in model._pending_sparse]
        res.append((loss.item(), model.flat.grad.clone(), sparse))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    assert model.g('tok.ns.kernel').abs().max().item() > 0
    for (k0, keys0, g0), (k1, keys1, g1) in zip(res[0][2], res[1][2]):
        assert k0 == k1 and torch.equal(keys0, keys1) and torch.equal(g0, g1)


def test_checkpoint_round_trip_and_refusals(dev, tmp_path):
    cfg = CONFIGS['d64_L4']()
    P, model, batch = setup(cfg, 9, dev)
    ns, seq, _ = batch
    tr = OneTransTrainer(cfg, model_dir=str(tmp_path), model=model)
    tr.train_step(batch)
    tr.save_model('g')
    with torch.no_grad():
        want = model((ns_t(ns, dev), ns_t(seq, dev)), training=False)
    other = OneTransTrainer(copy.deepcopy(cfg), model_dir=str(tmp_path), device=dev)
    other.load_model(str(tmp_path / 'g'))
    assert other.config.ns_tokenizer == 'group' and other.config.ns_token_groups == cfg.ns_token_groups
    with torch.no_grad():
        got = other.model((ns_t(ns, dev), ns_t(seq, dev)), training=False)
    for t in cfg.tasks:
        assert torch.equal(got[t], want[t])
    a, b = model.param_dict(), other.model.param_dict()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    weights = str(tmp_path / 'g' / 'model_weights.npz')
    # the other tokenizer mode, either way round
    cfg_a, Pa = NG.expand_to_auto(cfg, P)
    auto = OneTransModel(cfg_a, device=dev, init=Pa)
    before = auto.param_dict()
    with pytest.raises(ValueError, match="saved with ns_tokenizer='group'"):
        auto.load_weights(weights)
    after = auto.param_dict()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    auto.save_weights(str(tmp_path / 'auto.npz'))
    with pytest.raises(ValueError, match="saved with ns_tokenizer='auto'"):
        model.load_weights(str(tmp_path / 'auto.npz'))
    with pytest.raises(ValueError, match='another NS tokenizer mode'):
        model.load_param_dict({'tok.ns.kernel': Pa['tok.ns.kernel']})
    with pytest.raises(ValueError, match='another NS tokenizer mode'):
        auto.load_param_dict({'tok.ns.kernel': P['tok.ns.kernel']})
    # the same mode with other groups: the rows would mean other features
    cfg2 = copy.deepcopy(cfg)
    g = cfg2.ns_token_groups
    g[1], g[2] = g[2], g[1]
    with pytest.raises(ValueError, match='groups'):
        OneTransModel(cfg2, device=dev).load_weights(weights)


def test_an_auto_model_is_unchanged_by_a_group_model_next_to_it(dev):
    cfg_g = CONFIGS['d64_L4']()
    cfg_a = small_criteo('head')
    assert cfg_a.ns_tokenizer == 'auto'
    Pa, auto, batch = setup(cfg_a, 37, dev)
    ns, seq, lab = batch

    def logits():
        with torch.no_grad():
            auto((ns_t(ns, dev), ns_t(seq, dev)), training=False)
        return auto._last_logits.clone()

    before = logits()
    _, model, _ = setup(cfg_g, 37, dev)
    loss = keras_bce_loss(stack_labels(lab, cfg_g.tasks, dev),
                          model.forward_probs(ns_t(ns, dev), ns_t(seq, dev), training=True), cfg_g.tasks)
    loss.backward()
    assert torch.equal(before, logits())
