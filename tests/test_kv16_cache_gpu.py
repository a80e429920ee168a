"""GPU: the bf16 request cache of serving (DESIGN.md §7b "Cache precision").

Kernels against tests/kv16_ref.py: ot_kv_pack_bf16 bit for bit against the CPU rounding, ot_attn_fwd_cached_kv16
against the float64 attention over the rounded cache at the f32 cached kernel's own tolerances.  Server: the bf16
server equals the fp32 server run on a cache whose K/V columns were rounded (the emulation), through score, rank,
extend_requests (in place, reallocating, forking) and the inference engine."""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kv16_ref as KR
import rank_ref as RR
from recommend_amd import kernels as K
from recommend_amd._lib import OneTransHipError
from recommend_amd.data import make_batch, ragged_lengths
from recommend_amd.model import OneTransModel
from recommend_amd.params import init_params
from recommend_amd.serving import OneTransInferenceEngine, OneTransServer, bf16_cache_nbytes
from recommend_amd.span_block import span_forward
from test_model_gpu import ns_t, small_criteo
from test_padding_mask_gpu import MODEL_CASES

SENTINEL = 0x5A5A
REQ5 = np.array([0, 2, 1, 2, 0])


# =============================================================================== ot_kv_pack_bf16
@pytest.mark.parametrize('H,hd', [(2, 16), (2, 32)])
def test_pack(dev, H, hd):
    R_, rows, stride, row0 = 3, 13, 20, 5
    d = H * hd
    ld, ldc16 = 3 * d + 4, 2 * d + 8
    torch.manual_seed(3)
    src = torch.randn(R_ * rows, ld)
    special = KR.f32_from_bits([w for w, _ in KR.SPECIALS] + [0x7FC00000, 0x7F800001, 0xFFC12345])
    flat = src[:, d:3 * d].reshape(-1)
    where = torch.randperm(flat.numel())[:special.numel()]
    flat[where] = special
    src[:, d:3 * d] = flat.reshape(R_ * rows, 2 * d)
    dst = torch.full((R_ * stride, ldc16), SENTINEL, dtype=torch.int16).view(torch.bfloat16).to(dev)
    K.kv_pack_bf16(src.to(dev), ld, R_, rows, d, dst, ldc16, stride, row0)
    got = KR.bits16(dst.cpu()).reshape(R_, stride, ldc16)
    want = KR.round_bf16(src[:, d:3 * d]).reshape(R_, rows, 2 * d)
    win = got[:, row0:row0 + rows, :2 * d]
    nan = torch.isnan(want.float())
    assert int(nan.sum()) == 3
    assert torch.equal(win[~nan], KR.bits16(want)[~nan])                  # bit-equal to the CPU rounding
    assert torch.isnan(dst.cpu().reshape(R_, stride, ldc16)[:, row0:row0 + rows, :2 * d].float()[nan]).all()
    outside = torch.ones(R_, stride, ldc16, dtype=torch.bool)
    outside[:, row0:row0 + rows, :2 * d] = False
    assert (got[outside] == SENTINEL).all()                               # nothing else was written


# =============================================================================== ot_attn_fwd_cached_kv16
def cache_patterns(R_, Ic):
    """The three patterns of test_padding_mask_gpu.test_masked_cached_attention."""
    cv = np.ones((R_, max(Ic, 1)), bool)
    if Ic:
        cv[0, :33] = False                                  # crosses a key block
        cv[1, :] = False                                    # nothing cached is visible: the first block is all masked
        cv[2, 5:17] = False
    return cv


def run_attn(dev, hd, Ic, n, Kq, mask):
    R_, C, H = 3, 5, 2
    d = H * hd
    stride, ldc16 = Ic + 7, 2 * d + 8
    g = torch.Generator().manual_seed(1000 * hd + 10 * Ic + Kq)
    buf = torch.full((R_, stride, ldc16), float('nan'), dtype=torch.bfloat16)          # reserve rows and padding
    buf[:, :Ic, :2 * d] = KR.round_bf16(torch.randn(R_, Ic, 2 * d, generator=g))       # columns: never read
    own = torch.randn(C * n, 3 * d, generator=g)
    cv = cache_patterns(R_, Ic) if mask else None
    out = torch.full((C * Kq, d), float('nan'), device=dev)
    lse = torch.full((C * H * Kq,), float('nan'), device=dev)
    K.attn_fwd_cached_kv16(own.to(dev), 3 * d, buf.to(dev), ldc16, stride, torch.from_numpy(REQ5.astype(np.int32)).to(dev),
                           C, H, Ic, n, Kq, hd, out,
                           (torch.from_numpy(cv.astype(np.uint8)).to(dev), 0, cv.shape[1]) if mask else None, lse)
    ref, ref_lse = KR.cached_attention_ref(own, buf.reshape(R_ * stride, ldc16), stride, REQ5, H, Ic, n, Kq, d, cv)
    out, lse = out.double().cpu(), lse.double().cpu()
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    # the f32 cached kernel's own tolerances (test_masked_cached_attention), against the ROUNDED cache
    torch.testing.assert_close(out, ref.reshape(C * Kq, d), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse.reshape(C, H, Kq), ref_lse, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('hd', [16, 32, 64, 128])
@pytest.mark.parametrize('Ic', [0, 40, 64])
@pytest.mark.parametrize('Kq', [4, 1])
def test_attention_vs_float64(dev, Kq, Ic, hd, mask):
    """Ic = 40: a key block straddles cached and own rows; Ic = 64: the boundary falls on a block edge."""
    run_attn(dev, hd, Ic, 4, Kq, mask)


@pytest.mark.parametrize('mask', [False, True])
def test_attention_two_query_blocks(dev, mask):
    """n = Kq = 37: the shape extend_requests produces (two query blocks, causal among the own rows)."""
    run_attn(dev, 32, 40, 37, 37, mask)


# =============================================================================== server vs the emulation
REQ9 = torch.tensor([0, 1, 2, 2, 1, 0, 0, 1, 2])
SERVER_CASES = {
    'sep_d64_flat': lambda: small_criteo('tail'),
    'sep_d128_pyramid_masked': MODEL_CASES['sep_d128_pyramid'],
    'time_d128_masked': MODEL_CASES['time_d128'],
}
# max |Δp| between the bf16 server and the un-rounded fp32 server on these inputs, measured once on an MI355X
# (profiles/r10/serving_kv16.md); the test allows 4x, which only absorbs build-to-build summation-order changes
MEASURED_MAX_DP = {'sep_d64_flat': 4.861e-04, 'sep_d128_pyramid_masked': 3.089e-04, 'time_d128_masked': 2.049e-04}
_memo = {}


def round_cache(cache, d):
    """The emulation: an fp32 cache whose K | V columns hold bf16-representable values."""
    out = copy.copy(cache)
    out.layers = []
    for lay in cache.layers:
        kv = lay['kv']
        if kv is not None:
            kv = kv.clone()
            kv[:, d:] = kv[:, d:].bfloat16().float()
        out.layers.append({'Ic': lay['Ic'], 'kv': kv})
    return out


def probs(out, cfg):
    return np.stack([out[t].cpu().numpy()[:, 0] for t in cfg.tasks])


def served(dev, case):
    """One model per case and, computed once: the requests, the candidates and the three servers' scores."""
    if case in _memo:
        return _memo[case]
    cfg = SERVER_CASES[case]()
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    _, seq_r, _ = make_batch(3, cfg, seed=41)
    if getattr(cfg, 'seq_padding_mask', False):
        seq_r.update(ragged_lengths(3, cfg, seed=6))
    ns_c, _, _ = make_batch(9, cfg, seed=42)
    s = {'cfg': cfg, 'model': model, 'seq': seq_r, 'ns': ns_t(ns_c, dev), 'f32': OneTransServer(model),
         'b16': OneTransServer(model, 'bf16')}
    s['cache32'] = s['f32'].encode_requests(ns_t(seq_r, dev))
    s['cache16'] = s['b16'].encode_requests(ns_t(seq_r, dev))
    s['p32'] = probs(s['f32'].score(s['cache32'], REQ9, s['ns']), cfg)
    s['pemu'] = probs(s['f32'].score(round_cache(s['cache32'], cfg.hidden_dim), REQ9, s['ns']), cfg)
    s['p16'] = probs(s['b16'].score(s['cache16'], REQ9, s['ns']), cfg)
    _memo[case] = s
    return s


@pytest.mark.parametrize('case', list(SERVER_CASES))
def test_server_equals_emulation(dev, case):
    s = served(dev, case)
    print(f'{case}: max|p16 - pemu| = {np.abs(s["p16"] - s["pemu"]).max():.3e}, '
          f'max|p16 - p32| = {np.abs(s["p16"] - s["p32"]).max():.3e}')
    np.testing.assert_allclose(s['p16'], s['pemu'], atol=2e-6, rtol=0)     # the serving-vs-full-forward tolerance
    assert not np.array_equal(s['p16'], s['p32'])                          # the rounded route is really taken
    assert s['cache16'].dtype == 'bf16' and s['cache32'].dtype == 'fp32'


@pytest.mark.parametrize('case', list(SERVER_CASES))
def test_accuracy_cost(dev, case):
    """What the rounding costs against the un-rounded fp32 server (the yardstick is never the bf16 server)."""
    s = served(dev, case)
    dp = float(np.abs(s['p16'] - s['p32']).max())
    print(f'{case}: max |dp| bf16 cache vs fp32 cache = {dp:.3e}')
    assert 0 < dp <= 4 * MEASURED_MAX_DP[case]


# =============================================================================== append
def new_events(s, seed):
    """dL = 4 new events of the last sequence, all later than anything cached (with times under 'time')."""
    cfg = s['cfg']
    names = cfg.feature_config['sequence_features']
    rng = np.random.default_rng(seed)
    new = torch.from_numpy(rng.integers(0, cfg.seq_item_vocab, (3, 4)))
    if getattr(cfg, 'seq_fusion', 'sep') != 'time':
        return names[-1], new, None
    last = np.concatenate([s['seq'][n + '_time'] for n in names], axis=1).max(axis=1)
    return names[-1], new, torch.from_numpy(last[:, None] + np.array([[3, 1, 3, 2]]) + seed)


def extend(srv, cache, ev, dev):
    name, new, times = ev
    return srv.extend_requests(cache, name, new.to(dev), None if times is None else times.to(dev))


@pytest.mark.parametrize('case', ['sep_d64_flat', 'time_d128_masked'])
def test_append(dev, case):
    s = served(dev, case)
    cfg, f32, b16, ns = s['cfg'], s['f32'], s['b16'], s['ns']
    d = cfg.hidden_dim
    seq = ns_t(s['seq'], dev)
    ev1, ev2 = new_events(s, 5), new_events(s, 6)

    def emulate(ev):                                         # (c): round the cache, extend, round the appended rows
        return probs(f32.score(round_cache(extend(f32, round_cache(s['cache32'], d), ev, dev), d), REQ9, ns), cfg)

    c1, c2 = emulate(ev1), emulate(ev2)
    assert not np.array_equal(c1, c2) and not np.array_equal(c1, s['pemu'])
    # (a) room reserved: in place
    old = b16.encode_requests(seq, reserve=8)
    before = probs(b16.score(old, REQ9, ns), cfg)
    ptrs = [lay['kv16'].data_ptr() for lay in old.layers]
    ext_a = extend(b16, old, ev1, dev)
    assert [lay['kv16'].data_ptr() for lay in ext_a.layers] == ptrs
    assert all(a['kv16'] is o['kv16'] and a['high'] is o['high'] and a['Ic'] == o['Ic'] + 4 == a['high'][0]
               for a, o in zip(ext_a.layers, old.layers))
    a1 = probs(b16.score(ext_a, REQ9, ns), cfg)
    np.testing.assert_allclose(a1, c1, atol=2e-6, rtol=0)
    np.testing.assert_array_equal(probs(b16.score(old, REQ9, ns), cfg), before)      # the old cache is untouched
    # (b) no room: one reallocation of max(Ic + dL, 2 cap) rows
    tight = b16.encode_requests(seq)
    ext_b = extend(b16, tight, ev1, dev)
    assert all(b['kv16'].data_ptr() != t['kv16'].data_ptr() and b['cap'] == max(t['Ic'] + 4, 2 * t['cap'])
               for b, t in zip(ext_b.layers, tight.layers))
    np.testing.assert_allclose(probs(b16.score(ext_b, REQ9, ns), cfg), c1, atol=2e-6, rtol=0)
    np.testing.assert_allclose(probs(b16.score(ext_b, REQ9, ns), cfg), a1, atol=2e-6, rtol=0)
    assert ext_b.nbytes() == bf16_cache_nbytes(cfg, 3, ext_b.L_S, reserve=ext_b.layers[0]['cap'] - ext_b.L_S)
    # the same old cache a second time, other events: it no longer ends at the high-water mark, so it forks
    fork = extend(b16, old, ev2, dev)
    assert all(f['kv16'].data_ptr() != o['kv16'].data_ptr() for f, o in zip(fork.layers, old.layers))
    np.testing.assert_allclose(probs(b16.score(fork, REQ9, ns), cfg), c2, atol=2e-6, rtol=0)
    np.testing.assert_array_equal(probs(b16.score(ext_a, REQ9, ns), cfg), a1)        # the first extension stands
    np.testing.assert_array_equal(probs(b16.score(old, REQ9, ns), cfg), before)
    # the extension extends in place again while room is left (8 reserved, 4 + 4 used)
    ext_aa = extend(b16, ext_a, new_events(s, 20), dev)
    assert [lay['kv16'].data_ptr() for lay in ext_aa.layers] == ptrs


# =============================================================================== bytes
@pytest.mark.parametrize('case', list(SERVER_CASES))
def test_bytes(dev, case):
    s = served(dev, case)
    cfg = s['cfg']
    L_S = s['cache16'].L_S
    assert s['cache16'].nbytes() == bf16_cache_nbytes(cfg, 3, L_S)
    assert s['b16'].encode_requests(ns_t(s['seq'], dev), reserve=8).nbytes() == bf16_cache_nbytes(cfg, 3, L_S, reserve=8)
    held = [lay['kv'] for lay in s['cache32'].layers if lay['kv'] is not None]
    assert s['cache32'].nbytes() == sum(t.numel() * 4 for t in held) > 0
    assert 3 * s['cache16'].nbytes() == s['cache32'].nbytes()
    for lay in s['cache16'].layers:
        assert set(lay) == {'Ic', 'kv16', 'cap', 'high'}
        assert not any(isinstance(v, torch.Tensor) and v.dtype == torch.float32 for v in lay.values())
        assert lay['kv16'].dtype == torch.bfloat16 and tuple(lay['kv16'].shape) == (3, lay['cap'], 2 * cfg.hidden_dim)


# =============================================================================== rank and the engine
def test_rank(dev):
    s = served(dev, 'sep_d128_pyramid_masked')
    cfg, b16 = s['cfg'], s['b16']
    a = b16.rank(s['cache16'], REQ9, s['ns'], k=2)
    b = b16.rank(s['cache16'], REQ9, s['ns'], k=2)
    for key in ('index', 'score', 'count'):
        assert torch.equal(a[key], b[key])                                 # no atomics: bit-stable
    w = np.ones(len(cfg.tasks), np.float32)
    ridx, rsc, rcnt = RR.rank_topk(RR.fuse32(s['p16'], w, 'sum'), REQ9.numpy(), 3, 2)
    np.testing.assert_array_equal(a['index'].cpu().numpy(), ridx)
    np.testing.assert_array_equal(a['count'].cpu().numpy(), rcnt)
    np.testing.assert_array_equal(RR.bits(a['score'].cpu().numpy()), RR.bits(rsc))


def test_engine(dev, tmp_path):
    from recommend_amd.trainer import OneTransTrainer
    cfg = small_criteo('tail')
    cfg.max_seq_len = 12
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    OneTransTrainer(cfg, model_dir=str(tmp_path), model=OneTransModel(cfg, device=dev, init=P)).save_model('m')
    eng = OneTransInferenceEngine(str(tmp_path / 'm'), dev, cache_dtype='bf16')
    assert eng.server.cache_dtype == 'bf16'
    ns_c, seq, _ = make_batch(4, cfg, seed=9)
    names = list(ns_c)
    user = {k: ns_c[k][0] for k in names[:5]}
    cands = [{k: ns_c[k][i] for k in names[5:]} for i in range(4)]
    seq1 = {k: v[0][:n] for (k, v), n in zip(seq.items(), (3, 9, 5))}
    got = eng.score_candidates(user, seq1, cands)
    # the same user at the server level, through a server of its own
    cache, nsd = eng._one_request(user, seq1, cands)
    assert cache.dtype == 'bf16'
    srv = OneTransServer(eng.model, 'bf16')
    _, pre = eng.preprocess_input({}, {}, {}, seq1)
    want = srv.score(srv.encode_requests({k: torch.as_tensor(v[None]).to(dev) for k, v in pre.items()}),
                     torch.zeros(4, dtype=torch.int32), nsd)
    plain = OneTransInferenceEngine(str(tmp_path / 'm'), dev).score_candidates(user, seq1, cands)
    for t in cfg.tasks:
        for i in range(4):
            assert abs(got[i][t] - float(want[t][i, 0])) < 2e-6
    assert any(got[i][t] != plain[i][t] for i in range(4) for t in cfg.tasks)
    top = eng.rank_candidates(user, seq1, cands, k=2)
    assert len(top) == 2 and top[0][1] >= top[1][1]
    for i, _, p in top:
        assert all(abs(p[t] - got[i][t]) < 2e-6 for t in cfg.tasks)


# =============================================================================== refusals
def test_refusals(dev):
    s = served(dev, 'sep_d64_flat')
    cfg, model, f32, b16, ns = s['cfg'], s['model'], s['f32'], s['b16'], s['ns']
    with pytest.raises(ValueError, match='cache_dtype'):
        OneTransServer(model, 'fp16')
    with pytest.raises(ValueError, match='reserve'):
        b16.encode_requests(ns_t(s['seq'], dev), reserve=-1)
    ev = new_events(s, 5)
    for srv, cache in [(f32, s['cache16']), (b16, s['cache32'])]:
        with pytest.raises(ValueError, match='request cache was given'):
            srv.score(cache, REQ9, ns)
        with pytest.raises(ValueError, match='request cache was given'):
            srv.rank(cache, REQ9, ns, k=2)
        with pytest.raises(ValueError, match='request cache was given'):
            extend(srv, cache, ev, dev)
    lay = s['cache16'].layers[0]
    x = torch.zeros(9 * cfg.num_ns_tokens, cfg.hidden_dim, device=dev)
    with pytest.raises(ValueError, match='kv16'):
        span_forward(model, 0, x, 9, cfg.num_ns_tokens, cfg.num_ns_tokens, lay['Ic'], lay['Ic'] + cfg.num_ns_tokens,
                     cached=True, kv16=(lay['kv16'], lay['cap']), Ic=lay['Ic'], req=REQ9.to(dev, torch.int32), R=3,
                     for_backward=True)
    # the C ABI, each before any launch (the outputs keep their NaN)
    H, hd, Ic, n = 2, 32, 8, 4
    d = H * hd
    own = torch.randn(n, 3 * d, device=dev)
    req = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((n, d), float('nan'), device=dev)

    def attn(ldc16=2 * d, stride=Ic, hd_=hd, H_=H):
        buf = torch.zeros(max(stride, Ic) * max(ldc16, 2 * d), dtype=torch.bfloat16, device=dev)
        K.attn_fwd_cached_kv16(own, 3 * d, buf, ldc16, stride, req, 1, H_, Ic, n, n, hd_, out)

    for bad in (dict(ldc16=2 * d + 4), dict(ldc16=2 * d - 8), dict(stride=Ic - 1), dict(hd_=48, H_=1)):
        with pytest.raises(OneTransHipError):
            attn(**bad)
    dst = torch.zeros(Ic * (2 * d + 8), dtype=torch.bfloat16, device=dev)
    for ldc16, stride, row0 in [(2 * d + 4, n, 0), (2 * d - 8, n, 0), (2 * d, n - 1, 0), (2 * d, n, 1)]:
        with pytest.raises(OneTransHipError):
            K.kv_pack_bf16(own, 3 * d, 1, n, d, dst, ldc16, stride, row0)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not dst.float().any()
    attn()                                                   # and the accepted call writes every output
    assert not torch.isnan(out).any()
