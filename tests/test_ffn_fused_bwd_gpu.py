"""The fused FFN backward (gemm_ffn.hip ot_ffn_fused_bwd: FFN2 dgrad -> GELU' -> FFN1 dgrad + norm2 backward in one kernel,
split mode, d = 128) against the two launches it replaces, against float64, and its gate.

* against the unfused path (ot_mixed_gemm_rms_img twice, as model.py's block backward calls them) at 185 rows (B 5 x 37
  tokens: two tiles, the second partial, permuted rows and -1 padding), f 128 / 256 / 512, one and three weight
  groups, dropout 0 / 0.1, a tail map with Kq < I: dU and max |dU| bit for bit; dx1, dyo, dgamma, the rowabs parts and
  the dyo amax against the FFN1 dgrad launch fed the same dU within atol 1e-6 sqrt(f), no relative part (values of
  magnitude 4 to 12: the forward test's x2 tolerance, rtol 2e-5 and atol 2e-5 sqrt(f), holds twenty times over; the
  largest measured difference on these shapes is 4.0e-6, dgamma at f 512, 5.7 times under the bound, and every other
  figure is in profiles/r13/ffn_fused_bwd.md); the dropout masks of dyo identical.
* k permutation: exact small-integer operands with u >= 8, where gelu_erf_grad is exactly 1.0f (checked on the CPU with
  the project's formula in test_gelu_grad_is_one_from_8): dU and the GEMM2 sums are exact integers in both paths, and
  the epilogue is the same code over the same lanes in the same order, so dx1 / dyo / dgamma / rowabs / amax equal the
  unfused launch's bit for bit (that, not the float64 rounding bound, is what holds and is asserted).
* precision bar of tests/test_ffn_fused_gpu.py: max |fused - float64| <= 4 x max |native f32 - float64| (+ its floor) on
  dU and dx1 for the normal, outlier, near_eps and tiny_rows families of dy2 and for dy2 rows that are entirely zero.
* model level (2 layers, d 128, B 37): probs and every gradient bank against the float64 oracle with the switch on and
  off, new error <= 4 x old error + 8 ulp of the bank's scale; dropout 0 / 0.1, recompute, accumulate_grads; two runs
  with the switch on bit-identical.
* gate: with the switch off, d 64 / 256, bf16, fp8attn, fuse_bwd off or ONETRANS_PAIR_DGRAD=0 the launch list is the
  switched-off model's element for element and the bits are the same.
* CPU: a wrong struct_size, null operands and f not a multiple of 128 are refused with a message."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

from recommend_amd import _lib
from recommend_amd import kernels as K
from recommend_amd._lib import OT_EPI_DROPOUT, OT_EPI_GELU_BWD, OT_EPI_RMSNORM_BWD, OT_GEMM_NT
from recommend_amd.layout import IMAGE_UNIT_ELEMS, build_map

gpu = pytest.mark.gpu

D = 128
PAD = 5
EPS = 1e-6
M_ROWS = 185                       # B 5 x 37 tokens
TAIL = (37, 50)                    # Kq < I: the rows are the last 37 of a sample's 50 tokens
NEW_VS_OLD = 4.0


@pytest.fixture
def split_mode(dev):
    old = K.set_matmul_mode('split')
    prev = K.ffn_fused_bwd_on(-1)
    yield
    K.ffn_fused_bwd_on(prev)
    K.set_probe(None)
    K.set_matmul_mode(old)


def pair_image(W, dev):
    """W [G, N, K] (B[g][n][k]) -> the plain pair-form image (kscale_off -2), as the dgrad images are built."""
    G_, N, K_ = W.shape
    base = W.reshape(-1).float().to(dev)
    desc = torch.tensor([0, K_, 1, N * K_, -2, 0, 0, G_, N, K_], dtype=torch.int64, device=dev)
    units = G_ * (N // 128) * (K_ // 16)
    img = torch.zeros(units * IMAGE_UNIT_ELEMS, dtype=torch.int16, device=dev)
    K.split_images(base, desc, 1, units, img)
    return img


def row_map(rng, M, G):
    """M rows over G groups of uneven size (partial tiles with -1 entries); the same permuted rows in and out."""
    cuts = np.sort(rng.choice(np.arange(1, M), G - 1, replace=False)) if G > 1 else np.zeros(0, int)
    counts = np.diff(np.concatenate([[0], cuts, [M]])).astype(int)
    r = rng.permutation(M)
    per, o = [], 0
    for c in counts:
        per.append([r[o:o + c], r[o:o + c]])
        o += c
    return build_map(per)


def group_of_row(rm, M):
    g = np.zeros(M, int)
    rows = rm.rows[1]
    for t in range(rm.ntiles):
        rr = rows[t * 128:(t + 1) * 128]
        g[rr[rr >= 0]] = int(rm.tile_group[t])
    return torch.as_tensor(g)


def nan(dev, *shape):
    return torch.full(shape, float('nan'), device=dev)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def device_ops(dev, rm, dy2, u, x1, dres, gamma, W2, W1):
    """W2 [G, f, D] (the FFN2 dgrad's B[g][n = f][k = d]), W1 [G, D, f] (the FFN1 dgrad's B[g][n = d][k = f])."""
    x1 = x1.float()
    rstd = torch.rsqrt((x1.double() ** 2).mean(1) + EPS).float()
    o = dict(rm=rm, d=rm.to(dev), dy2=dy2.float().to(dev), u=u.float().to(dev), x1=x1.to(dev),
             dres=dres.float().to(dev) if dres is not None else None, gamma=gamma.float().to(dev), rstd=rstd.to(dev),
             W2=W2.float().to(dev), W1=W1.float().to(dev), img2=pair_image(W2, dev), img1=pair_image(W1, dev))
    rmax = torch.empty(dy2.shape[0], 1, device=dev)
    K.rows_absmax(o['dy2'], D, dy2.shape[0], D, rmax)
    o['rmax'] = rmax
    return o


_OPS = {}


def operands(dev, f, G):
    """Seeded operands of one shape, built once and shared (never written by a test)."""
    key = (f, G)
    if key not in _OPS:
        M = M_ROWS
        rng = np.random.default_rng(11 * f + G)
        gen = torch.Generator().manual_seed(f + G)
        dy2 = torch.randn(M, D, generator=gen) * 10.0 ** (-2 * torch.rand(M, 1, generator=gen))
        _OPS[key] = device_ops(dev, row_map(rng, M, G), dy2, 1.5 * torch.randn(M, f, generator=gen),
                               torch.randn(M, D, generator=gen), torch.randn(M, D, generator=gen),
                               1 + 0.1 * torch.randn(D, generator=gen),
                               torch.randn(G, f, D, generator=gen) / math.sqrt(f),
                               torch.randn(G, D, f, generator=gen) / math.sqrt(D))
    return _OPS[key]


def outputs(dev, M, f, drop):
    return dict(du=nan(dev, M + PAD, f), dx1=nan(dev, M + PAD, D), dyo=nan(dev, M + PAD, D) if drop > 0 else None,
                dg=torch.zeros(D, device=dev), b_du=torch.zeros(1, device=dev), b_dyo=torch.zeros(1, device=dev),
                rm_dyo=nan(dev, M + PAD, 1))


def run_fused(dev, o, f, G, drop, tail=TAIL, seed=1234, site=3):
    rm, d, M = o['rm'], o['d'], o['dy2'].shape[0]
    r = outputs(dev, M, f, drop)
    K.ffn_fused_bwd(o['dy2'], D, o['rmax'], 1, d['rows'][1], d['tile_group'], rm.ntiles, o['img2'], G, o['img1'], G, f,
                    o['u'], f, r['du'], f, o['x1'], D, o['gamma'], o['rstd'], r['dx1'], D, r['dg'], du_amax=r['b_du'],
                    dres=o['dres'], lddres=D, dx_masked=r['dyo'], lddxm=D, amax_out=r['b_dyo'], rowabs_out=r['rm_dyo'],
                    rowabs_n=1, seed=seed, site=site, drop=drop, tail=tail, device=dev)
    torch.cuda.synchronize()
    return r


def run_unfused(dev, o, f, G, drop, tail=TAIL, seed=1234, site=3, images=True, du_in=None):
    """The FFN2 and FFN1 dgrad launches of the block backward (split mode: pair images and dU's row maxima between
    them; ``images`` False: no images, whatever arithmetic the current mode runs; ``du_in``: only the FFN1 dgrad, fed
    this dU and its row maxima)."""
    rm, d, M = o['rm'], o['d'], o['dy2'].shape[0]
    nt = f // 128
    r = outputs(dev, M, f, drop)
    rm_du = nan(dev, M + PAD, nt)
    if du_in is None:
        kw2 = dict(bimg=(o['img2'], nt, 0), a_rowmax=o['rmax'], a_rowmax_n=1, amax_out=r['b_du'], rowabs_out=rm_du,
                   rowabs_n=nt) if images else {}
        K.gemm_rms(OT_GEMM_NT, o['dy2'], D, D, d['rows'][1], o['W2'], f * D, D, f, d['tile_group'], rm.ntiles, r['du'],
                   f, d['rows'][1], epi=OT_EPI_GELU_BWD, aux=o['u'], ldaux=f, device=dev, **kw2)
    else:
        r['du'] = du_in
        rm_du[:M] = du_in[:M].reshape(M, nt, 128).abs().amax(2)
    kw1 = dict(bimg=(o['img1'], 1, 0), a_rowmax=rm_du, a_rowmax_n=nt, amax_out=r['b_dyo'], rowabs_out=r['rm_dyo'],
               rowabs_n=1) if images else {}
    K.gemm_rms(OT_GEMM_NT, r['du'], f, f, d['rows'][1], o['W1'], D * f, f, D, d['tile_group'], rm.ntiles, r['dx1'], D,
               d['rows'][1], epi=OT_EPI_RMSNORM_BWD | (OT_EPI_DROPOUT if drop > 0 else 0), seed=seed, site=site,
               drop=drop, tail=tail, nx=o['x1'], ldnx=D, ngamma=o['gamma'], nrstd=o['rstd'], dres=o['dres'], lddres=D,
               dx_masked=r['dyo'], lddxm=D, dgamma=r['dg'], accumulate_dgamma=False, device=dev, **kw1)
    torch.cuda.synchronize()
    return r


# ------------------------------------------------------------------------------------------------ CPU
def erf_project(a):
    """one_plus_erf of csrc/common.h in float32 steps (each fma as a float64 product and sum rounded once to f32)."""
    f32 = np.float32
    fma = lambda x, y, z: f32(np.float64(x) * np.float64(y) + np.float64(z))
    x = f32(min(max(f32(a), f32(-4)), f32(4)))
    x2 = f32(x * x)
    p = f32(-2.72614225801306e-10)
    for c in (2.77068142495902e-08, -2.10102402082508e-06, -5.69250639462346e-05, -7.34990630326855e-04,
              -2.95459980854025e-03, -1.60960333262415e-02):
        p = fma(p, x2, f32(c))
    q = f32(-1.45660718464996e-05)
    for c in (-2.13374055278905e-04, -1.68282697438203e-03, -7.37332916720468e-03, -1.42647390514189e-02):
        q = fma(q, x2, f32(c))
    return fma(f32(x * p), f32(f32(1) / q), f32(1))


def test_gelu_grad_is_one_from_8():
    """gelu_erf_grad(u) = fma(u c, exp2(-k u^2), 0.5 (1 + erf(u / sqrt 2))) is exactly 1.0f for u >= 8: the argument of
    erf is clamped to 4, where 1 + erf evaluates to exactly 2 with a correctly rounded reciprocal (the device's
    v_rcp_f32 may be one ulp off: that it gives 2 as well is what the GPU test's exact dU shows), and
    u c exp2(-k u^2) <= 8 x 0.4 x 2^-46 is far below half an ulp of 1."""
    f32 = np.float32
    for u in (8.0, 9.5, 13.0, 40.0):
        assert erf_project(f32(u) * f32(0.70710678118654752440)) == f32(2.0)
        t = f32(f32(f32(-0.72134752044448170368) * f32(u)) * f32(u))
        small = np.float64(f32(u) * f32(0.39894228040143267794)) * 2.0 ** np.float64(t) * 1.01
        assert small < 2.0 ** -26
        assert f32(small + np.float64(f32(0.5) * f32(2.0))) == f32(1.0)


def bwd_args(**kw):
    a = _lib.FfnFusedBwdArgs()
    a.struct_size = ctypes.sizeof(_lib.FfnFusedBwdArgs)
    for k in ('dy2', 'dy2_rowmax', 'u', 'du', 'w2_image', 'w1_image', 'x1', 'gamma', 'rstd', 'dx1', 'dgamma',
              'workspace'):
        setattr(a, k, 4096)                      # never dereferenced: validation fails before any launch
    a.lddy2 = a.ldx1 = a.lddx1 = 128
    a.ldu = a.lddu = 512
    a.f, a.ntiles, a.dy2_rowmax_n, a.w1_groups, a.w2_groups, a.ws_bytes = 512, 1, 1, 1, 1, 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')
def test_bad_arguments_are_refused():
    with pytest.raises(_lib.OneTransHipError, match='null arguments'):
        _lib.call('ot_ffn_fused_bwd', None, None)
    a = bwd_args()
    a.struct_size -= 8
    with pytest.raises(_lib.OneTransHipError, match='struct_size'):
        _lib.call('ot_ffn_fused_bwd', ctypes.byref(a), None)
    for k in ('dy2', 'dy2_rowmax', 'u', 'du', 'w2_image', 'w1_image', 'x1', 'dx1', 'dgamma'):
        with pytest.raises(_lib.OneTransHipError, match='null operand'):
            _lib.call('ot_ffn_fused_bwd', ctypes.byref(bwd_args(**{k: None})), None)
    for f in (0, 64, 192, 2048):
        with pytest.raises(_lib.OneTransHipError, match='bad sizes'):
            _lib.call('ot_ffn_fused_bwd', ctypes.byref(bwd_args(f=f)), None)
    with pytest.raises(_lib.OneTransHipError, match='dx_masked'):
        _lib.call('ot_ffn_fused_bwd', ctypes.byref(bwd_args(drop_rate=0.1, tail_K=1, tail_I=1)), None)
    with pytest.raises(_lib.OneTransHipError, match='workspace too small'):
        _lib.call('ot_ffn_fused_bwd', ctypes.byref(bwd_args(ws_bytes=16)), None)
    assert _lib.size('ot_ffn_fused_bwd_on', -1) in (0, 1)


# ------------------------------------------------------------------------------------------------ kernel level
@gpu
def test_k_permutation_exact_integers(dev, split_mode):
    """Exact-integer operands (see the module docstring): dU exact against float64, everything else bit for bit."""
    f, M, G = 512, M_ROWS, 3
    rng = np.random.default_rng(5)
    rm = row_map(rng, M, G)
    g = group_of_row(rm, M).numpy()
    dy2 = rng.integers(-3, 4, (M, D)).astype(np.float64)
    mult = np.repeat(np.array([1, 4, 1, 8]), 128)                       # per chunk: the row's chunk scales differ
    W2 = rng.integers(-2, 3, (G, f, D)).astype(np.float64) * mult[None, :, None]
    W1 = rng.integers(-2, 3, (G, D, f)).astype(np.float64)
    u = 8.0 + 4.0 * rng.random((M, f))
    dU = np.einsum('mk,mfk->mf', dy2, W2[g])                             # gelu'(u) == 1 here
    assert np.abs(dU).max() < 2 ** 13
    assert np.einsum('mf,mnf->mn', np.abs(dU), np.abs(W1[g])).max() < 2 ** 24
    t = torch.as_tensor
    gen = torch.Generator().manual_seed(3)
    o = device_ops(dev, rm, t(dy2), t(u), torch.randn(M, D, generator=gen), torch.randn(M, D, generator=gen),
                   1 + 0.1 * torch.randn(D, generator=gen), t(W2), t(W1))
    for drop in (0.0, 0.1):
        a, b = run_fused(dev, o, f, G, drop), run_unfused(dev, o, f, G, drop)
        assert torch.equal(a['du'][:M].double().cpu(), t(dU)) and torch.isnan(a['du'][M:]).all()
        assert a['b_du'].item() == np.abs(dU).max()
        for k in ('du', 'dx1', 'dyo', 'dg', 'b_du', 'b_dyo', 'rm_dyo'):
            if a[k] is not None:
                assert same_bits(a[k], b[k]), f'{k} (drop {drop}) differs from the unfused launches'


@gpu
@pytest.mark.parametrize('drop', [0.0, 0.1])
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('f', [128, 256, 512])
def test_against_unfused(dev, split_mode, f, G, drop):
    M = M_ROWS
    o = operands(dev, f, G)
    a = run_fused(dev, o, f, G, drop)
    b = run_unfused(dev, o, f, G, drop)
    assert same_bits(a['du'], b['du']), 'dU differs from the FFN2 dgrad launch'
    assert same_bits(a['b_du'], b['b_du']) and a['b_du'].item() > 0
    assert not torch.isnan(a['du'][:M]).any() and torch.isnan(a['du'][M:]).all()   # every mapped row stored, no other
    assert not torch.isnan(a['dx1'][:M]).any() and torch.isnan(a['dx1'][M:]).all()
    c = run_unfused(dev, o, f, G, drop, du_in=a['du'])                   # the FFN1 dgrad launch fed the same dU
    tol = dict(rtol=0.0, atol=1e-6 * math.sqrt(f))
    names = ['dx1', 'dg', 'rm_dyo', 'b_dyo'] + (['dyo'] if drop > 0 else [])
    for k in names:
        n = M if a[k].shape[0] == M + PAD else a[k].shape[0]
        diff = (a[k][:n] - c[k][:n]).abs().max().item()
        print(f'ffn_fused_bwd f{f} G{G} drop{drop} {k}: max |diff| {diff:.3e}  (scale {c[k][:n].abs().max().item():.2e})')
    for k in names:
        n = M if a[k].shape[0] == M + PAD else a[k].shape[0]
        torch.testing.assert_close(a[k][:n], c[k][:n], **tol)
        assert torch.isnan(a[k][n:]).all()
    if drop > 0:
        za, zc = a['dyo'][:M] == 0, c['dyo'][:M] == 0
        assert torch.equal(za, zc), 'dropout mask differs'
        assert 0.05 < za.float().mean().item() < 0.15
    again = run_fused(dev, o, f, G, drop)
    for k in names + ['du', 'b_du']:
        assert same_bits(a[k], again[k]), f'{k}: two runs differ'


def gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


@gpu
@pytest.mark.parametrize('case', ['normal', 'outlier', 'near_eps', 'tiny_rows', 'zero_rows'])
def test_precision_bar(dev, split_mode, case):
    """Against float64, beside the native f32 MFMA path (two launches, no images) on the same operands; no residual
    gradient, so the FFN branch's own error is what is compared."""
    f, M, G = 512, M_ROWS, 3
    gen = torch.Generator().manual_seed(f + len(case))
    rng = np.random.default_rng(len(case))
    rm = row_map(rng, M, G)
    g = group_of_row(rm, M)
    A = torch.randn(M, D, generator=gen, dtype=torch.float64)
    if case == 'outlier':
        A[torch.arange(M), torch.randint(0, D, (M,), generator=gen)] *= 1e4
    elif case == 'near_eps':
        A *= 1e-4
    elif case == 'tiny_rows':
        A[::2] *= 1e-4
    elif case == 'zero_rows':
        A[::3] = 0.0
    dy2 = A.float()
    u = (1.5 * torch.randn(M, f, generator=gen, dtype=torch.float64)).float()
    x1 = torch.randn(M, D, generator=gen, dtype=torch.float64).float()
    gamma = (1 + 0.1 * torch.randn(D, generator=gen, dtype=torch.float64)).float()
    W2 = (torch.randn(G, f, D, generator=gen, dtype=torch.float64) / math.sqrt(f)).float()
    W1 = (torch.randn(G, D, f, generator=gen, dtype=torch.float64) / math.sqrt(D)).float()
    o = device_ops(dev, rm, dy2, u, x1, None, gamma, W2, W1)
    r = o['rstd'].double().cpu()[:, None]
    dU = torch.einsum('mk,mfk->mf', dy2.double(), W2.double()[g]) * gelu_grad64(u.double())
    gv = torch.einsum('mf,mnf->mn', dU, W1.double()[g]) * gamma.double()
    ref = gv * r - x1.double() * (r ** 3 * (gv * x1.double()).sum(1, keepdim=True) / D)
    a = run_fused(dev, o, f, G, 0.0, (1, 1))
    old = K.set_matmul_mode('f32')
    try:
        b = run_unfused(dev, o, f, G, 0.0, (1, 1), images=False)
    finally:
        K.set_matmul_mode(old)
    assert torch.isfinite(a['dx1'][:M]).all() and torch.isfinite(a['du'][:M]).all()
    if case == 'zero_rows':
        assert (a['du'][:M][::3] == 0).all() and (a['dx1'][:M][::3] == 0).all()
    for k, want in (('du', dU), ('dx1', ref)):
        e_pair = (a[k][:M].double().cpu() - want).abs().max().item()
        e_f32 = (b[k][:M].double().cpu() - want).abs().max().item()
        scale = want.abs().max().item()
        floor = 8 * 2.0 ** -24 * scale
        print(f'ffn_fused_bwd f{f} {case} {k}: pair {e_pair:.3e}  f32 {e_f32:.3e}  '
              f'ratio {e_pair / max(e_f32, 1e-300):.2f}  (scale {scale:.2e})')
        assert e_pair <= NEW_VS_OLD * e_f32 + floor, f'{case} {k}: fused {e_pair:.3e} > {NEW_VS_OLD} x f32 {e_f32:.3e}'


# ------------------------------------------------------------------------------------------------ model level
def model_cfg(d=128, H=4, dropout=0.0, **kw):
    from recommend_amd.config import workload_config
    cfg = workload_config('C2')
    cfg.hidden_dim, cfg.num_heads, cfg.ffn_dim, cfg.num_layers, cfg.num_ns_tokens = d, H, 2 * d, 2, 12
    cfg.sparse_features = {k: 40 + 7 * i for i, k in enumerate(cfg.sparse_features)}
    cfg.seq_item_vocab = 300
    cfg._seq_lens = [20, 20, 20]
    cfg.dropout_rate = dropout
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def ns_t(dct, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dct.items()}


B_MODEL = 37
_ORACLE = {}


def oracle(cfg, key, P, batch, seed):
    """The float64 oracle's probs and gradients (computed once per configuration and dropout seed)."""
    from oracle import onetrans_ref as R
    k = key + (seed,)
    if k not in _ORACLE:
        ns, seq, lab = batch
        rl, rg, rout = R.loss_and_grads(R.to_torch(P), cfg, R.to_torch(ns), R.to_torch(seq), R.to_torch(lab),
                                        training=True, seed=seed)
        _ORACLE[k] = (torch.stack([rout['probs'][t].reshape(-1) for t in cfg.tasks]), rg)
    return _ORACLE[k]


def run_model(cfg, dev, P, batch, on, accumulate=False, fuse_bwd=None):
    """One forward_probs + backward with the switch ``on``; returns (probs, {bank: grad}, seed, launch list)."""
    from recommend_amd.model import OneTransModel, keras_bce_loss
    from recommend_amd.trainer import stack_labels
    K.ffn_fused_bwd_on(int(on))
    ns, seq, lab = batch
    model = OneTransModel(cfg, device=str(dev), init=P)
    if fuse_bwd is not None:
        model.fuse_bwd = fuse_bwd
    model.accumulate_grads = accumulate
    model.flat.grad.fill_(1.0 if accumulate else float('nan'))
    probe = K.Probe()
    K.set_probe(probe)
    probs = model.forward_probs(ns_t(ns, dev), ns_t(seq, dev), training=True)
    seed = (model.dropout_seed + 0x9E3779B9 * model._step) & 0xFFFFFFFF
    keras_bce_loss(stack_labels(lab, cfg.tasks, dev), probs, cfg.tasks).backward()
    torch.cuda.synchronize()
    K.set_probe(None)
    grads = {n: model.g(n).detach().clone() for n in model.layout.shapes}
    return probs.detach().clone(), grads, seed, [f'{r[0]} {r[4]}' for r in probe.recs]


def errors(probs, grads, ref_probs, ref_grads, minus=0.0):
    out = {'probs': ((probs.double().cpu() - ref_probs).abs().max().item(), 1.0)}
    for name, r in ref_grads.items():
        if name not in grads:
            continue
        g = grads[name].double().cpu() - minus
        if name == 'tok.ns.kernel':
            g = g[:r.shape[0]]
        out[name] = ((g.reshape(r.shape) - r).abs().max().item(), r.abs().max().item())
    return out


@gpu
@pytest.mark.parametrize('variant', ['plain', 'accumulate', 'recompute'])
@pytest.mark.parametrize('dropout', [0.0, 0.1])
def test_model_precision_bar(dev, split_mode, dropout, variant):
    from recommend_amd.data import make_batch
    from recommend_amd.params import init_params
    cfg = model_cfg(dropout=dropout, recompute_blocks=variant == 'recompute')
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    batch = make_batch(B_MODEL, cfg, seed=1000)
    acc = variant == 'accumulate'
    p1, g1, seed, lab1 = run_model(cfg, dev, P, batch, True, acc)
    p1b, g1b, _, _ = run_model(cfg, dev, P, batch, True, acc)
    p0, g0, seed0, lab0 = run_model(cfg, dev, P, batch, False, acc)
    assert seed == seed0
    assert sum('ffn_fused_bwd' in s for s in lab1) == cfg.num_layers and not any('ffn_fused_bwd' in s for s in lab0)
    assert len(lab1) == len(lab0) - cfg.num_layers                       # one launch fewer per block
    assert same_bits(p1, p1b), 'probs differ between two runs'
    for n in g1:
        assert same_bits(g1[n], g1b[n]), f'{n}: two runs differ'
    rp, rg = oracle(cfg, (dropout,), P, batch, seed)
    e1 = errors(p1, g1, rp, rg, 1.0 if acc else 0.0)
    e0 = errors(p0, g0, rp, rg, 1.0 if acc else 0.0)
    for n in e1:
        (a, scale), (b, _) = e1[n], e0[n]
        floor = 8 * 2.0 ** -24 * max(scale, 1.0 if acc else 0.0)
        print(f'drop{dropout} {variant} {n}: fused {a:.3e}  old {b:.3e}  ratio {a / max(b, 1e-300):.2f}  '
              f'(scale {scale:.2e})')
        assert math.isfinite(a)
        assert a <= NEW_VS_OLD * b + floor, f'{n}: fused error {a:.3e} > {NEW_VS_OLD} x old {b:.3e}'


GATE_CASES = {
    'd64': dict(cfg=dict(d=64)),
    'd256': dict(cfg=dict(d=256)),
    'bf16': dict(cfg=dict(compute_dtype='bf16')),
    'fp8attn': dict(cfg=dict(H=2, compute_dtype='fp8attn')),
    'fuse_bwd_off': dict(fuse_bwd=False),
    'pair_dgrad_off': dict(env={'ONETRANS_PAIR_DGRAD': '0'}),
}


@gpu
@pytest.mark.parametrize('name', list(GATE_CASES))
def test_gate_false_runs_the_old_launches(dev, split_mode, monkeypatch, name):
    from recommend_amd.data import make_batch
    from recommend_amd.params import init_params
    case = GATE_CASES[name]
    for k, v in case.get('env', {}).items():
        monkeypatch.setenv(k, v)
    cfg = model_cfg(**case.get('cfg', {}))
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    batch = make_batch(B_MODEL, cfg, seed=1000)
    p1, g1, _, lab1 = run_model(cfg, dev, P, batch, True, fuse_bwd=case.get('fuse_bwd'))
    p0, g0, _, lab0 = run_model(cfg, dev, P, batch, False, fuse_bwd=case.get('fuse_bwd'))
    assert not any('ffn_fused_bwd' in s for s in lab1)
    assert lab1 == lab0 and len(lab1) > 0
    assert same_bits(p1, p0)
    for n in g1:
        assert same_bits(g1[n], g0[n]), n


@gpu
def test_switch_off_is_the_two_launches(dev, split_mode):
    """Inside the gate with the switch off: no fused call, the FFN2 and FFN1 dgrad launches, two runs bit-identical."""
    from recommend_amd.data import make_batch
    from recommend_amd.params import init_params
    cfg = model_cfg(dropout=0.1)
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    batch = make_batch(B_MODEL, cfg, seed=1000)
    p0, g0, _, lab0 = run_model(cfg, dev, P, batch, False)
    p0b, g0b, _, lab0b = run_model(cfg, dev, P, batch, False)
    assert not any('ffn_fused_bwd' in s for s in lab0) and lab0 == lab0b
    assert sum(f'epi{OT_EPI_GELU_BWD} ' in s for s in lab0) == cfg.num_layers
    assert same_bits(p0, p0b)
    for n in g0:
        assert same_bits(g0[n], g0b[n]), n
