"""GPU: the key-padding mask (``seq_padding_mask``) — the masked attention kernels and
ot_seq_key_valid against float64, the masked model against tests/padmask_ref.py (and the untouched oracle on
un-padded histories), padding inertness, recompute, cached serving and the refusals.

Bounds: the kernels' are tests/test_kernels_gpu.py::test_attention's, the model's tests/test_model_gpu.py's (logits
LOGIT_TOL, gradients 2e-4 of the gradient's scale), serving's tests/test_serving_gpu.py's."""

import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd._lib import OneTransHipError
from recommend_amd.data import make_batch, ragged_lengths
from recommend_amd.model import OneTransModel, keras_bce_loss
from recommend_amd.params import init_params
from recommend_amd.serving import OneTransServer
from recommend_amd.trainer import OneTransTrainer, stack_labels
from oracle import onetrans_np as RN
from oracle import onetrans_ref as R

import padmask_ref as PM
from test_model_gpu import LOGIT_TOL, ns_t, small_criteo, with_dropout

B_MODEL = 37


# =============================================================================== kernels vs float64
def patterns(B, I):
    """Validity patterns [B, I] (bool), named: all valid; a padding prefix of 33 (crosses a 32-key block); only the
    last 4 valid; two padded segments in the 'sep' shape [pad real SEP pad real NS..]."""
    out = {'all': np.ones((B, I), bool)}
    p = np.ones((B, I), bool); p[:, :min(33, I - 1)] = False
    out['prefix33'] = p
    p = np.zeros((B, I), bool); p[:, I - 4:] = True
    out['last4'] = p
    p = np.ones((B, I), bool)
    a, b = I // 3, I // 3 + 1 + I // 2                      # segment ends: [0, a) [SEP a] [a + 1, b) then valid tokens
    for s in range(B):
        p[s, :max(0, a - 1 - s)] = False                    # sample s keeps 1 + s events of the first segment
        p[s, a + 1:b - 2 * s - 1] = False
    out['two_segments'] = p
    return out


def attn_masked_ref(qkv, B, H, I, qpos, hd, valid):
    """Float64: queries at qpos [B, K] over all I keys; key j visible to query i iff j <= i and (valid j or j == i).
    Returns (out [B*K, d], lse [B, H, K])."""
    d = H * hd
    Kq = qpos.shape[1]
    bi = torch.arange(B)[:, None]
    q = qkv[:, :d].reshape(B, I, H, hd)[bi, qpos]
    k = qkv[:, d:2 * d].reshape(B, I, H, hd)
    v = qkv[:, 2 * d:].reshape(B, I, H, hd)
    s = torch.einsum('bqhd,bkhd->bhqk', q, k) / math.sqrt(hd)
    kpos = torch.arange(I)[None, None, :]
    vis = (kpos <= qpos[:, :, None]) & (valid[:, None, :] | (kpos == qpos[:, :, None]))       # [B, K, I]
    s = torch.where(vis[:, None], s, torch.tensor(-math.inf, dtype=s.dtype))
    out = torch.einsum('bhqk,bkhd->bqhd', torch.softmax(s, -1), v).reshape(B * Kq, d)
    return out, torch.logsumexp(s, -1)


def run_masked(dev, B, H, I, Kq, hd, valid, qpos=None, backward=True, seed=0):
    torch.manual_seed(seed)
    d = H * hd
    qkv = torch.randn(B * I, 3 * d, dtype=torch.float64)
    qkv_d = qkv.float().to(dev)
    # the mask as a layer reads it: the last I columns of a wider array (pointer offset, row stride)
    wide = torch.zeros(B, I + 5, dtype=torch.uint8)
    wide[:, 5:] = torch.from_numpy(valid.astype(np.uint8))
    kv = (wide.to(dev), 5, I + 5)
    qp = torch.arange(I - Kq, I)[None].expand(B, Kq) if qpos is None else torch.from_numpy(qpos)
    qp_d = None if qpos is None else torch.from_numpy(qpos.astype(np.int32).reshape(-1)).to(dev)
    out = torch.full((B * Kq, d), float('nan'), device=dev)
    lse = torch.full((B * H * Kq,), float('nan'), device=dev)
    K.attn_fwd_masked(qkv_d, 3 * d, B, H, I, Kq, hd, out, lse, kv, qpos=qp_d)
    qkv_r = qkv.clone().requires_grad_(True)
    ref, ref_lse = attn_masked_ref(qkv_r, B, H, I, qp, hd, torch.from_numpy(valid))
    torch.testing.assert_close(out.double().cpu(), ref.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse.double().cpu().reshape(B, H, Kq), ref_lse.detach(), rtol=1e-5, atol=1e-5)
    # a padding query sees itself and the valid keys before it: with none before it, its output is its own v
    v = qkv[:, 2 * d:].reshape(B, I, d)
    for b in range(B):
        for j in range(Kq):
            p = int(qp[b, j])
            if not valid[b, :p].any():
                torch.testing.assert_close(out[b * Kq + j].double().cpu(), v[b, p], rtol=1e-6, atol=1e-6)
    if not backward:
        return
    dout = torch.randn(B * Kq, d, dtype=torch.float64)
    ref.backward(dout)
    dqkv = torch.full((B * I, 3 * d), float('nan'), device=dev)
    if Kq < I:
        dqkv[:, :d].zero_()
    K.attn_bwd_masked(qkv_d, 3 * d, out, dout.float().to(dev), lse, B, H, I, Kq, hd, dqkv, kv, qpos=qp_d)
    torch.testing.assert_close(dqkv.double().cpu(), qkv_r.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('hd', [32, 64, 16, 128])
@pytest.mark.parametrize('I', [37, 70])
@pytest.mark.parametrize('Kq', ['I', 9, 3, 1])
def test_masked_attention(dev, hd, I, Kq):
    """Forward (out, lse) and backward (dqkv), every row compared, padding queries included: the MFMA kernels
    (K > 4; head_dim 64 backward as two 32-dim waves), the short-tail kernels (K = 3: KQ 4; K = 1: KQ 1; at
    head_dim 16 the forward stays on the MFMA kernel)."""
    B, H = 3, 2
    Kq = I if Kq == 'I' else Kq
    for name, valid in patterns(B, I).items():
        run_masked(dev, B, H, I, Kq, hd, valid)


@pytest.mark.parametrize('hd', [16, 128])
def test_masked_attention_forward_other_head_dims(dev, hd):
    for name, valid in patterns(3, 70).items():
        run_masked(dev, 3, 2, 70, 70, hd, valid, backward=False)


def test_masked_attention_selected_queries(dev):
    """Queries at per-sample kept positions (the SEL backward, the forward's per-query positions), at every head_dim."""
    B, H, I, Kq = 3, 2, 70, 23
    rng = np.random.default_rng(4)
    qpos = np.stack([np.append(np.sort(rng.choice(I - 1, Kq - 1, replace=False)), I - 1) for _ in range(B)])
    for hd in (32, 16, 64, 128):
        for name, valid in patterns(B, I).items():
            run_masked(dev, B, H, I, Kq, hd, valid, qpos=qpos)


def test_masked_attention_refuses_bf16(dev):
    qkv = torch.zeros(8, 3 * 64, device=dev)
    out, lse = torch.zeros(8, 64, device=dev), torch.zeros(2 * 8, device=dev)
    kv = (torch.ones(1, 8, dtype=torch.uint8, device=dev), 0, 8)
    with K.precision('bf16'):
        with pytest.raises(OneTransHipError):
            K.attn_fwd_masked(qkv, 3 * 64, 1, 2, 8, 8, 32, out, lse, kv)
        with pytest.raises(OneTransHipError):
            K.attn_bwd_masked(qkv, 3 * 64, out, out, lse, 1, 2, 8, 8, 32, torch.zeros_like(qkv), kv)


@pytest.mark.parametrize('Ic', [0, 40])
@pytest.mark.parametrize('Kq', [4, 1])
def test_masked_cached_attention(dev, Ic, Kq):
    """The cached forward: candidates' N rows over their request's cached rows under cache_valid, own rows valid; at
    every head_dim."""
    for hd in (32, 16, 64, 128):
        check_masked_cached(dev, Ic, Kq, hd)


def check_masked_cached(dev, Ic, Kq, hd):
    R_, C, H, n = 3, 5, 2, 4
    d = H * hd
    torch.manual_seed(1)
    req = np.array([0, 2, 1, 2, 0])
    cache = torch.randn(R_ * max(Ic, 1), 3 * d, dtype=torch.float64)
    own = torch.randn(C * n, 3 * d, dtype=torch.float64)
    cv = np.ones((R_, max(Ic, 1)), bool)
    if Ic:
        cv[0, :33] = False                                  # crosses a key block
        cv[1, :] = False                                    # nothing cached is visible: the first block is all masked
        cv[2, 5:17] = False
    out = torch.full((C * Kq, d), float('nan'), device=dev)
    lse = torch.full((C * H * Kq,), float('nan'), device=dev)
    K.attn_fwd_cached_masked(own.float().to(dev), 3 * d, (cache.float().to(dev), d) if Ic else None, 3 * d,
                             torch.from_numpy(req.astype(np.int32)).to(dev), C, H, Ic, n, Kq, hd, out,
                             (torch.from_numpy(cv.astype(np.uint8)).to(dev), 0, cv.shape[1]) if Ic else None, lse)
    # reference: each candidate's [cached rows ; own rows] as one sequence of Ic + n tokens, the last Kq queries
    I = Ic + n
    full = torch.cat([torch.cat([cache.view(R_, -1, 3 * d)[req[c], :Ic], own.view(C, n, 3 * d)[c]]) for c in range(C)])
    valid = np.concatenate([cv[req][:, :Ic], np.ones((C, n), bool)], 1)
    qp = torch.arange(I - Kq, I)[None].expand(C, Kq)
    ref, ref_lse = attn_masked_ref(full, C, H, I, qp, hd, torch.from_numpy(valid))
    torch.testing.assert_close(out.double().cpu(), ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse.double().cpu().reshape(C, H, Kq), ref_lse, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('fusion', ['sep', 'time'])
def test_seq_key_valid(dev, fusion):
    """ot_seq_key_valid == the numpy builder; out-of-range lengths clamp on the device."""
    cfg = masked(small_criteo('tail'), fusion)
    B = 11
    _, seq, _ = make_batch(B, cfg, seed=7)
    lens = ragged_lengths(B, cfg, seed=3)
    first = cfg.feature_config['sequence_features'][0] + '_len'
    lens[first][3], lens[first][4] = -2, 100
    names, caps, offs, L_S = PM.seq_layout(cfg, seq)
    L0 = L_S + cfg.num_ns_tokens
    rank = None
    if fusion == 'time':
        import time_fusion_ref as TF
        rank = torch.from_numpy(TF.merge_ranks([seq[n + '_time'] for n in names]).astype(np.int32)).to(dev)
    lens_d = torch.from_numpy(np.stack([lens[n + '_len'] for n in names]).astype(np.int32)).to(dev)
    got = torch.full((B, L0), 7, dtype=torch.uint8, device=dev)
    K.seq_key_valid(lens_d, caps, offs, B, L0, got, rank=rank)
    np.testing.assert_array_equal(got.cpu().numpy(), PM.valid0_np(cfg, seq, lens))


# =============================================================================== model vs padmask_ref
def masked(cfg, fusion='sep', dropout=False):
    cfg.seq_padding_mask = True
    cfg.seq_fusion = fusion
    if dropout:
        with_dropout(cfg)
    return cfg


MODEL_CASES = {
    'sep_d64': lambda: masked(small_criteo('tail')),
    'sep_d128_pyramid': lambda: masked(small_criteo('tail', pyramid=True, layers=3, d=128, H=4, f=256, Lns=12,
                                                    seq_lens=(20, 20, 20))),
    'd256_hd64_pyramid': lambda: masked(small_criteo('tail', pyramid=True, layers=2, d=256, H=4, f=1024, Lns=4,
                                                     seq_lens=(12, 9, 7))),
    'time_d128': lambda: masked(small_criteo('tail', d=128, H=4, f=256, Lns=12, seq_lens=(20, 20, 20)), 'time'),
    'sep_d64_dropout': lambda: masked(small_criteo('head', pyramid=True, layers=3), dropout=True),
}


def setup_masked(cfg, B, dev, seed=0):
    P = init_params(cfg, cfg.ns_input_width(), seed=seed, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    ns, seq, lab = make_batch(B, cfg, seed=1000)             # full-length arrays: whatever sits before the real events
    lens = ragged_lengths(B, cfg, seed=11)                   # is padding content (under 'time': with arbitrary times)
    return P, model, (ns, seq, lab), lens


def run_model(model, cfg, ns, seq, lens, lab, dev, training):
    model.flat.grad.fill_(float('nan'))
    probs = model.forward_probs(ns_t(ns, dev), ns_t({**seq, **lens}, dev), training=training)
    seed = (model.dropout_seed + 0x9E3779B9 * model._step) & 0xFFFFFFFF if training else 0
    loss = keras_bce_loss(stack_labels(lab, cfg.tasks, dev), probs, cfg.tasks)
    loss.backward()
    torch.cuda.synchronize()
    return loss, seed


@pytest.mark.parametrize('case', list(MODEL_CASES))
def test_model_matches_masked_reference(dev, case):
    """Logits, loss, every dense gradient and the table gradients vs the float64 masked reference."""
    cfg = MODEL_CASES[case]()
    training = cfg.dropout_rate > 0
    P, model, (ns, seq, lab), lens = setup_masked(cfg, B_MODEL, dev)
    loss, seed = run_model(model, cfg, ns, seq, lens, lab, dev, training)
    rl, rg, rout = PM.loss_and_grads(R.to_torch(P), cfg, R.to_torch(ns), R.to_torch(seq), lens, R.to_torch(lab),
                                     training=training, seed=seed)
    for t in cfg.tasks:
        lg = model._last_logits[cfg.tasks.index(t)].detach().double().cpu().numpy()
        np.testing.assert_allclose(lg, rout['logits'][t].detach().numpy()[:, 0], atol=LOGIT_TOL, rtol=0)
    assert abs(loss.item() - rl.item()) < 1e-4
    for name in model.layout.shapes:
        g = model.g(name).double().cpu()
        r = rg[name]
        if name == 'tok.ns.kernel':
            assert torch.all(g[r.shape[0]:] == 0)
            g = g[:r.shape[0]]
        err = (g.reshape(r.shape) - r).abs().max().item() / max(1e-3, r.abs().max().item())
        assert err < 2e-4, f'{name}: rel err {err:.2e}'
    for (tname, keys, grads) in model._pending_sparse:
        dense = torch.zeros(rg[tname].shape, dtype=torch.float64)
        dense.index_add_(0, keys.cpu(), grads.double().cpu())
        assert (dense - rg[tname]).abs().max().item() / max(1e-3, rg[tname].abs().max().item()) < 2e-4, tname


def test_model_matches_truncated_oracle_and_differs_from_unmasked(dev):
    """The masked model on padded samples == the untouched oracle on each sample's un-padded history (tail groups, no
    pruning), and it is not today's forward: the un-masked model on the same batch differs by more than 1e-2."""
    cfg = MODEL_CASES['sep_d64']()
    P, model, (ns, seq, _), lens = setup_masked(cfg, B_MODEL, dev)
    plain = copy.deepcopy(cfg)
    plain.seq_padding_mask = False
    with torch.no_grad():
        model((ns_t(ns, dev), ns_t({**seq, **lens}, dev)), training=False)
        got = model._last_logits.double().cpu().numpy()
        unmasked = OneTransModel(plain, device=dev, init=P)
        unmasked((ns_t(ns, dev), ns_t(seq, dev)), training=False)
        other = unmasked._last_logits.double().cpu().numpy()
    for b in range(B_MODEL):
        ns1, seq1 = PM.truncate(cfg, ns, seq, lens, b)
        ref = RN.forward(P, plain, ns1, seq1)
        for ti, t in enumerate(cfg.tasks):
            assert abs(got[ti, b] - float(np.asarray(ref['logits'][t]).reshape(-1)[0])) < LOGIT_TOL, (b, t)
    assert np.abs(got - other).max() > 1e-2


# =============================================================================== padding is inert
def garbage_padding(cfg, seq, lens, seed=9):
    rng = np.random.default_rng(seed)
    out = dict(seq)
    for n, L in zip(cfg.feature_config['sequence_features'], cfg._seq_lens):
        pad = np.arange(L)[None, :] < L - lens[n + '_len'][:, None]
        out[n] = np.where(pad, rng.integers(0, cfg.seq_item_vocab, size=seq[n].shape), seq[n])
    return out


@pytest.mark.parametrize('case', ['sep_d128_pyramid', 'time_d128'])
def test_padding_content_is_inert(dev, case):
    """Other ids in the padding: logits and gradients stay within the parity bounds."""
    cfg = MODEL_CASES[case]()
    P, model, (ns, seq, lab), lens = setup_masked(cfg, B_MODEL, dev)
    run_model(model, cfg, ns, seq, lens, lab, dev, False)
    lg0 = model._last_logits.detach().clone()
    g0 = {n: model.g(n).clone() for n in model.layout.shapes}
    run_model(model, cfg, ns, garbage_padding(cfg, seq, lens), lens, lab, dev, False)
    assert (model._last_logits.detach() - lg0).abs().max().item() <= LOGIT_TOL
    for n in g0:
        err = (model.g(n) - g0[n]).abs().max().item() / max(1e-3, g0[n].abs().max().item())
        assert err < 2e-4, (n, err)


def test_train_step_leaves_padding_only_rows(dev):
    """After one train_step the emb.seq_item rows that only padding positions reference keep their bits, weight and
    Adagrad accumulator: every gradient through a padding row is a product with an exact zero."""
    cfg = MODEL_CASES['sep_d64']()
    P, model, (ns, seq, lab), lens = setup_masked(cfg, B_MODEL, dev)
    # padding positions reference ids from the upper half of the vocabulary, real events the lower half
    half = cfg.seq_item_vocab // 2
    seq = {n: v % half for n, v in seq.items()}
    pad_ids = []
    for n, L in zip(cfg.feature_config['sequence_features'], cfg._seq_lens):
        pad = np.arange(L)[None, :] < L - lens[n + '_len'][:, None]
        seq[n] = np.where(pad, half + seq[n], seq[n])
        pad_ids.append(seq[n][pad])
    pad_ids = np.unique(np.concatenate(pad_ids))
    assert len(pad_ids) > 3
    tr = OneTransTrainer(cfg, model=model)
    w0 = model.tables['emb.seq_item'].clone()
    tr.train_step((ns, {**seq, **lens}, lab))
    torch.cuda.synchronize()
    w1 = model.tables['emb.seq_item']
    idx = torch.from_numpy(pad_ids).to(dev)
    assert torch.equal(w1[idx].view(torch.int32), w0[idx].view(torch.int32))
    real = torch.from_numpy(np.unique(np.concatenate([v[v < half] for v in seq.values()]))).to(dev)
    assert not torch.equal(w1[real], w0[real])               # the step did train the table
    acc = tr.optimizer.acc['emb.seq_item']
    a0 = torch.full_like(acc[:1], float(cfg.adagrad_initial_accumulator))
    assert torch.equal(acc[idx].view(torch.int32), a0.expand(len(idx), -1).contiguous().view(torch.int32))
    assert not torch.equal(acc[real], a0.expand(len(real), -1))


# =============================================================================== recompute
def test_recompute_is_bit_identical(dev):
    cfg = MODEL_CASES['sep_d64_dropout']()
    P, model, (ns, seq, lab), lens = setup_masked(cfg, B_MODEL, dev)
    run_model(model, cfg, ns, seq, lens, lab, dev, True)
    g0 = {n: model.g(n).clone() for n in model.layout.shapes}
    s0 = [(t, k.clone(), g.clone()) for (t, k, g) in model._pending_sparse]
    cfg2 = copy.deepcopy(cfg)
    cfg2.recompute_blocks = True
    m2 = OneTransModel(cfg2, device=dev, init=P)
    assert m2.recompute
    run_model(m2, cfg2, ns, seq, lens, lab, dev, True)
    for n in g0:
        assert torch.equal(g0[n], m2.g(n)), n
    for (ta, ka, ga), (tb, kb, gb) in zip(s0, m2._pending_sparse):
        assert ta == tb and torch.equal(ka, kb) and torch.equal(ga, gb)


# =============================================================================== serving
@pytest.mark.parametrize('case', ['sep_d64', 'sep_d128_pyramid', 'time_d128'])
def test_serving_matches_masked_model(dev, case):
    cfg = MODEL_CASES[case]()
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    Rq, C = 5, 23
    _, seq_r, _ = make_batch(Rq, cfg, seed=2000)
    seq_r.update(ragged_lengths(Rq, cfg, seed=4))
    ns_c, _, _ = make_batch(C, cfg, seed=3000)
    req = np.random.default_rng(1).integers(0, Rq, C)
    req[:Rq] = np.arange(Rq)
    srv = OneTransServer(model)
    cache = srv.encode_requests(ns_t(seq_r, dev))
    assert cache.valid.shape == (Rq, cache.L_S) and cache.valid.dtype == torch.uint8
    got = srv.score(cache, torch.from_numpy(req), ns_t(ns_c, dev))
    full = {k: v[req] for k, v in seq_r.items()}
    with torch.no_grad():
        ref = model((ns_t(ns_c, dev), ns_t(full, dev)), training=False)
    for t in cfg.tasks:
        np.testing.assert_allclose(got[t].cpu().numpy(), ref[t].cpu().numpy(), atol=2e-6, rtol=0)


def test_extend_requests_matches_reencode(dev):
    cfg = MODEL_CASES['sep_d64']()
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    Rq, C, dL = 3, 9, 4
    _, seq_r, _ = make_batch(Rq, cfg, seed=41)
    lens = ragged_lengths(Rq, cfg, seed=6)
    ns_c, _, _ = make_batch(C, cfg, seed=42)
    last = cfg.feature_config['sequence_features'][-1]
    new = np.random.default_rng(5).integers(0, cfg.seq_item_vocab, (Rq, dL))
    full = {**seq_r, **lens}
    full[last] = np.concatenate([seq_r[last], new], 1)
    full[last + '_len'] = lens[last + '_len'] + dL
    req = torch.tensor([0, 1, 2, 2, 1, 0, 0, 1, 2])
    srv = OneTransServer(model)
    ext = srv.extend_requests(srv.encode_requests(ns_t({**seq_r, **lens}, dev)), last, torch.from_numpy(new).to(dev))
    ref_cache = srv.encode_requests(ns_t(full, dev))
    assert ext.L_S == ref_cache.L_S and torch.equal(ext.valid, ref_cache.valid)
    a = srv.score(ext, req, ns_t(ns_c, dev))
    b = srv.score(ref_cache, req, ns_t(ns_c, dev))
    for t in cfg.tasks:
        np.testing.assert_allclose(a[t].cpu().numpy(), b[t].cpu().numpy(), atol=2e-6, rtol=0)


# =============================================================================== refusals
def test_refusals(dev):
    base = MODEL_CASES['sep_d64']
    for field, value, err in [('compute_dtype', 'bf16', NotImplementedError),
                              ('compute_dtype', 'fp8attn', NotImplementedError),
                              ('pyramid_select', 'norm', ValueError)]:
        cfg = base()
        setattr(cfg, field, value)
        if value == 'norm':
            cfg.pyramid_enabled = True
        with pytest.raises(err):
            OneTransModel(cfg, device=dev)
    cfg = base()
    P, model, (ns, seq, lab), lens = setup_masked(cfg, 5, dev)
    with pytest.raises(ValueError):                          # a missing length
        model.forward_probs(ns_t(ns, dev), ns_t(seq, dev), training=False)
    bad = {k: v.copy() for k, v in lens.items()}
    next(iter(bad.values()))[0] = 99
    with pytest.raises(ValueError):                          # a host array out of range
        model.forward_probs(ns_t(ns, dev), {**ns_t(seq, dev), **bad}, training=False)
    # a device tensor is not read back: out-of-range values clamp on the device
    full = {k: np.full_like(v, 10 ** 6) for k, v in lens.items()}
    capped = {n + '_len': np.full(5, L, np.int64) for n, L in zip(cfg.feature_config['sequence_features'], cfg._seq_lens)}
    with torch.no_grad():
        a = model.forward_probs(ns_t(ns, dev), ns_t({**seq, **full}, dev), training=False).clone()
        b = model.forward_probs(ns_t(ns, dev), ns_t({**seq, **capped}, dev), training=False)
    assert torch.equal(a, b)
    from recommend_amd.data import make_request_batch
    ns4, seq4, lab4, req = make_request_batch(2, 3, cfg, seed=1)
    seq4.update(ragged_lengths(2, cfg, seed=2))
    with pytest.raises(NotImplementedError):                 # request-grouped training: 4-tuple batches
        OneTransTrainer(cfg, model=model).train_step((ns4, seq4, lab4, req))


def test_inference_engine_supplies_lengths(dev, tmp_path):
    """The engine pads every history to max_seq_len and, with the switch on, supplies the lengths: single, batch and
    two-stage inference agree, and equal the un-masked model on the un-padded histories (tail groups, no pruning)."""
    from recommend_amd.serving import OneTransInferenceEngine
    cfg = MODEL_CASES['sep_d64']()
    cfg.max_seq_len = 12
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    tr = OneTransTrainer(cfg, model_dir=str(tmp_path), model=OneTransModel(cfg, device=dev, init=P))
    tr.save_model('m')
    eng = OneTransInferenceEngine(str(tmp_path / 'm'), device=dev)
    assert eng.config.seq_padding_mask is True and eng.config.seq_len_suffix == '_len'
    ns_c, seq, _ = make_batch(4, cfg, seed=9)
    names = list(ns_c)
    user = {k: ns_c[k][0] for k in names[:5]}
    cands = [{k: ns_c[k][i] for k in names[5:]} for i in range(4)]
    seq1 = {k: v[0][:n] for (k, v), n in zip(seq.items(), (3, 9, 0))}     # one user's histories: 3, 9 and no events
    pre = eng.preprocess_input(user, cands[0], {}, seq1)[1]
    assert {k: int(v) for k, v in pre.items() if k.endswith('_len')} == {k + '_len': n for k, n in
                                                                         zip(seq, (3, 9, 0))}
    got = eng.batch_inference([(user, c, {}, seq1) for c in cands])
    single = eng.single_inference(user, cands[2], {}, seq1)
    fast = eng.score_candidates(user, seq1, cands)
    plain = copy.deepcopy(cfg)
    plain.seq_padding_mask = False
    ns4 = {**{k: np.repeat(v.reshape(1, -1), 4, 0) for k, v in user.items()},
           **{k: ns_c[k] for k in names[5:]}}
    ref = RN.forward(P, plain, ns4, {k: np.repeat(v[None], 4, 0) for k, v in seq1.items()})
    for t in cfg.tasks:
        assert abs(single[t] - got[2][t]) < 2e-6
        for i in range(4):
            assert abs(fast[i][t] - got[i][t]) < 2e-6
            assert abs(got[i][t] - float(np.asarray(ref['probs'][t]).reshape(-1)[i])) < LOGIT_TOL / 4
