"""The fused FFN forward (gemm_ffn.hip ot_ffn_fused_fwd: FFN1 -> GELU -> FFN2 in one kernel, split mode, d = 128) against
the two launches it replaces, against float64, and its switch.

* k permutation (GEMM2 reads its B operand from GEMM1's accumulators, whose k order inside a 16-k step is permuted):
  exact small-integer operands against numpy float64.  x1 in 0..3, W1 in 0..2 times a per-chunk factor (so a row's
  chunk scales differ and the rescale of the running sums runs), b1 = 8, rstd = 1, gamma = 1: every u is an integer
  >= 8, where gelu_erf(u) == u exactly (erf saturates at 1 in f32), W2 in -2..2: every product and partial sum is an
  integer below 2^24, so U and x2 must equal the float64 result exactly.
* against the unfused path (ot_mixed_gemm_rms_img twice, as model.py's block forward calls them): U and max |U| bit for
  bit, x2 / rstd within the plane-vs-staged tolerance (rtol 2e-5, atol 2e-5 sqrt(K), K = f), the dropout mask identical
  (a dropped element leaves x2 == x1 exactly), rows the map does not name unstored; without u_out the same x2 bits.
* precision bar of tests/test_pair_precision_gpu.py: max |fused - float64| <= 4 x max |native f32 - float64| (+ its
  floor) on that file's adversarial row families and rows whose GELU sits at the 0.17 floor.
* the switch: off, the model's block forward makes no fused call and is the two-launch path; on, it makes them."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd._lib import (OT_AX_GELU, OT_AX_RMSNORM, OT_EPI_BIAS, OT_EPI_DROPOUT, OT_EPI_RESIDUAL,
                                OT_EPI_ROW_RSTD, OT_GEMM_NT)
from recommend_amd.layout import IMAGE_UNIT_ELEMS, build_map

D = 128
PAD = 5
EPS = 1e-6
PAIR_VS_F32 = 4.0


@pytest.fixture(autouse=True)
def split_mode(dev):
    old = K.set_matmul_mode('split')
    prev = K.ffn_fused(-1)
    yield
    K.ffn_fused(prev)
    K.set_matmul_mode(old)


def pair_image(W, dev, gamma=None):
    """W [G, N, K] (B[g][n][k]) -> the pair-form image (gamma folded, or plain: kscale_off -2)."""
    G_, N, K_ = W.shape
    base = torch.cat([W.reshape(-1), gamma if gamma is not None else torch.zeros(0)]).float().to(dev)
    desc = torch.tensor([0, K_, 1, N * K_, G_ * N * K_ if gamma is not None else -2, 0, 0, G_, N, K_],
                        dtype=torch.int64, device=dev)
    units = G_ * (N // 128) * (K_ // 16)
    img = torch.zeros(units * IMAGE_UNIT_ELEMS, dtype=torch.int16, device=dev)
    K.split_images(base, desc, 1, units, img)
    return img


def row_map(rng, M, G):
    """M rows over G groups of uneven size (a partial last tile and -1 entries per group); the same permuted rows as
    input and output rows, as the block forward's tail map."""
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


_OPS = {}


def operands(dev, f, M, G):
    """Seeded operands of one shape, built once and shared (never written by a test)."""
    key = (f, M, G)
    if key not in _OPS:
        rng = np.random.default_rng(7 * f + M + G)
        gen = torch.Generator().manual_seed(f + M + G)
        rm = row_map(rng, M, G)
        x1 = torch.randn(M, D, generator=gen)
        x1 *= 10.0 ** (-2 * torch.rand(M, 1, generator=gen))           # rows of different magnitude
        W1 = torch.randn(G, f, D, generator=gen) / math.sqrt(D)
        W2 = torch.randn(G, D, f, generator=gen) / math.sqrt(f)
        gamma = 1 + 0.1 * torch.randn(D, generator=gen)
        o = dict(rm=rm, d=rm.to(dev), x1=x1.to(dev), W1=W1.to(dev), W2=W2.to(dev), gamma=gamma.to(dev),
                 rstd=torch.rsqrt((x1 * x1).mean(1) + EPS).to(dev),
                 b1=(0.5 * torch.randn(G, f, generator=gen)).to(dev), b2=(0.1 * torch.randn(G, D, generator=gen)).to(dev),
                 img1=pair_image(W1, dev, gamma), img2=pair_image(W2, dev))
        _OPS[key] = o
    return _OPS[key]


def run_fused(dev, o, f, M, G, drop, tail, with_u=True, seed=1234, site=3):
    rm, d = o['rm'], o['d']
    x2, rstd_out = nan(dev, M + PAD, D), nan(dev, M + PAD)
    u = nan(dev, M + PAD, f) if with_u else None
    amax = torch.zeros(1, device=dev)
    K.ffn_fused_fwd(o['x1'], D, d['rows'][1], d['tile_group'], rm.ntiles, o['rstd'], o['img1'], G, o['img2'], G,
                    o['b1'], f, o['b2'], D, f, x2, D, u_out=u, ldu=f, u_amax=amax, rstd_out=rstd_out, eps=EPS,
                    seed=seed, site=site, drop=drop, tail=tail)
    torch.cuda.synchronize()
    return x2, rstd_out, u, amax


def run_unfused(dev, o, f, M, G, drop, tail, seed=1234, site=3, images=True):
    """The FFN1 and FFN2 launches of the block forward (split mode: pair images and the row maxima between them;
    ``images`` False: no images, whatever arithmetic the current mode runs)."""
    rm, d = o['rm'], o['d']
    nt = f // 128
    u, umax = nan(dev, M + PAD, f), nan(dev, M + PAD, nt)
    x2, rstd_out = nan(dev, M + PAD, D), nan(dev, M + PAD)
    amax = torch.zeros(1, device=dev)
    kw1 = dict(bimg=(o['img1'], nt, 0), rowmax_out=umax, rowmax_n=nt, amax_out=amax) if images else {}
    K.gemm_rms(OT_GEMM_NT, o['x1'], D, D, d['rows'][1], o['W1'], D * f, D, f, d['tile_group'], rm.ntiles, u, f,
               d['rows'][1], a_xform=OT_AX_RMSNORM, rstd=o['rstd'], gamma=o['gamma'], bias=o['b1'], bias_gstride=f,
               epi=OT_EPI_BIAS, device=dev, **kw1)
    kw2 = dict(bimg=(o['img2'], 1, 0), a_rowmax=umax, a_rowmax_n=nt) if images else {}
    K.gemm_rms(OT_GEMM_NT, u, f, f, d['rows'][1], o['W2'], f * D, f, D, d['tile_group'], rm.ntiles, x2, D,
               d['rows'][1], a_xform=OT_AX_GELU, bias=o['b2'], bias_gstride=D,
               epi=OT_EPI_BIAS | OT_EPI_RESIDUAL | (OT_EPI_DROPOUT if drop > 0 else 0) | OT_EPI_ROW_RSTD,
               res=o['x1'], ldres=D, res_tok=0, seed=seed, site=site, drop=drop, tail=tail, rstd_out=rstd_out,
               eps=EPS, device=dev, **kw2)
    torch.cuda.synchronize()
    return x2, rstd_out, u, amax


def test_k_permutation_exact_integers(dev):
    """Exact-integer operands against numpy float64 (see the module docstring): U and x2 exact."""
    f, M, G = 512, 300, 3
    rng = np.random.default_rng(5)
    rm = row_map(rng, M, G)
    g = group_of_row(rm, M).numpy()
    x1 = rng.integers(0, 4, (M, D)).astype(np.float64)
    mult = np.repeat(np.array([1, 4, 1, 2]), 128)                        # per chunk: the row's chunk scales differ
    W1 = rng.integers(0, 3, (G, f, D)).astype(np.float64) * mult[None, :, None]
    W2 = rng.integers(-2, 3, (G, D, f)).astype(np.float64)
    b1 = np.full((G, f), 8.0)
    b2 = rng.integers(-3, 4, (G, D)).astype(np.float64)
    U = np.einsum('mk,mfk->mf', x1, W1[g]) + b1[g]
    assert U.min() >= 8 and U.max() < 2 ** 13
    X2 = x1 + np.einsum('mf,mnf->mn', U, W2[g]) + b2[g]                  # gelu(u) == u here
    assert np.abs(np.einsum('mf,mnf->mn', U, np.abs(W2[g]))).max() < 2 ** 24
    t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)
    o = dict(rm=rm, d=rm.to(dev), x1=t(x1), rstd=torch.ones(M, device=dev), b1=t(b1), b2=t(b2),
             img1=pair_image(t(W1).cpu(), dev, torch.ones(D)), img2=pair_image(t(W2).cpu(), dev))
    x2, _, u, amax = run_fused(dev, o, f, M, G, 0.0, (1, 1))
    assert torch.equal(u[:M].double().cpu(), torch.as_tensor(U))
    assert torch.equal(x2[:M].double().cpu(), torch.as_tensor(X2))
    assert amax.item() == U.max()
    assert torch.isnan(x2[M:]).all() and torch.isnan(u[M:]).all()


@pytest.mark.parametrize('drop', [0.0, 0.1])
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('M', [96, 300])
@pytest.mark.parametrize('f', [128, 256, 512])
def test_against_unfused(dev, f, M, G, drop):
    o = operands(dev, f, M, G)
    tail = (12, 20)                                                      # K < I: rows are 12 of a sample's 20 tokens
    x2, rstd, u, amax = run_fused(dev, o, f, M, G, drop, tail)
    x2r, rstdr, ur, amaxr = run_unfused(dev, o, f, M, G, drop, tail)
    assert not torch.isnan(x2[:M]).any() and torch.isnan(x2[M:]).all()   # every mapped row stored, no other
    assert not torch.isnan(u[:M]).any() and torch.isnan(u[M:]).all()
    assert torch.isnan(rstd[M:]).all()
    du = (u[:M] - ur[:M]).abs().max().item()
    dx = (x2[:M] - x2r[:M]).abs().max().item()
    print(f'f{f} M{M} G{G} drop{drop}: max |dU| {du:.3e}  max |dx2| {dx:.3e}  '
          f'max |drstd| {(rstd[:M] - rstdr[:M]).abs().max().item():.3e}')
    assert same_bits(u, ur), 'U differs from the FFN1 launch'
    assert same_bits(amax, amaxr) and amax.item() > 0
    torch.testing.assert_close(x2[:M], x2r[:M], rtol=2e-5, atol=2e-5 * math.sqrt(f))
    torch.testing.assert_close(rstd[:M], rstdr[:M], rtol=2e-5, atol=2e-5 * math.sqrt(f))
    kept, keptr = x2[:M] != o['x1'], x2r[:M] != o['x1']
    assert torch.equal(kept, keptr), 'dropout mask differs'
    if drop > 0:
        assert 0.05 < 1.0 - kept.float().mean().item() < 0.15
    # no u_out: the same x2 / rstd bits
    x2n, rstdn, _, amaxn = run_fused(dev, o, f, M, G, drop, tail, with_u=False)
    assert same_bits(x2n, x2) and same_bits(rstdn, rstd) and same_bits(amaxn, amax)


def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


@pytest.mark.parametrize('case', ['normal', 'outlier', 'near_eps', 'tiny_rows', 'gelu_floor'])
def test_precision_bar(dev, case):
    """Against float64, beside the native f32 MFMA path (two launches, no images) on the same operands."""
    f, M, G = 512, 600, 3
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
    x1 = A.float()
    W1 = (torch.randn(G, f, D, generator=gen, dtype=torch.float64) / math.sqrt(D)).float()
    W2 = (torch.randn(G, D, f, generator=gen, dtype=torch.float64) / math.sqrt(f)).float()
    gamma = (1 + 0.1 * torch.randn(D, generator=gen, dtype=torch.float64)).float()
    b1 = (0.1 * torch.randn(G, f, generator=gen, dtype=torch.float64)).float()
    if case == 'gelu_floor':
        b1 = b1 - 6.0                                                    # every u < 0: gelu(u) in [-0.17, 0)
    b2 = (0.1 * torch.randn(G, D, generator=gen, dtype=torch.float64)).float()
    rstd = (1.0 / torch.sqrt((x1.double() ** 2).mean(1) + EPS)).float()
    u64 = torch.einsum('mk,mfk->mf', x1.double() * rstd.double()[:, None] * gamma.double(), W1.double()[g])
    u64 += b1.double()[g]
    if case == 'gelu_floor':
        assert u64.max().item() < 0
    ref = x1.double() + torch.einsum('mf,mnf->mn', gelu64(u64), W2.double()[g]) + b2.double()[g]
    o = dict(rm=rm, d=rm.to(dev), x1=x1.to(dev), W1=W1.to(dev), W2=W2.to(dev), gamma=gamma.to(dev), rstd=rstd.to(dev),
             b1=b1.to(dev), b2=b2.to(dev), img1=pair_image(W1, dev, gamma), img2=pair_image(W2, dev))
    xp = run_fused(dev, o, f, M, G, 0.0, (1, 1))[0]
    old = K.set_matmul_mode('f32')
    try:
        xf = run_unfused(dev, o, f, M, G, 0.0, (1, 1), images=False)[0]
    finally:
        K.set_matmul_mode(old)
    assert torch.isfinite(xp[:M]).all()
    # the FFN branch alone (the residual x1 is added exactly by both): its error against its own scale
    e_pair = (xp[:M].double().cpu() - ref).abs().max().item()
    e_f32 = (xf[:M].double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    floor = 8 * 2.0 ** -24 * scale
    print(f'ffn_fused f{f} {case}: pair {e_pair:.3e}  f32 {e_f32:.3e}  ratio {e_pair / max(e_f32, 1e-300):.2f}  '
          f'(scale {scale:.2e})')
    assert e_pair <= PAIR_VS_F32 * e_f32 + floor, f'{case}: fused error {e_pair:.3e} > {PAIR_VS_F32} x f32 {e_f32:.3e}'


def test_switch(dev, monkeypatch):
    """Off: the block forward makes no fused call (the two launches: the parent's path, bit for bit over two runs);
    on: one fused call per block, and the loss agrees with the two-launch path's."""
    from recommend_amd.config import workload_config
    from recommend_amd.data import make_batch
    from recommend_amd.model import OneTransModel
    from recommend_amd.params import init_params
    from recommend_amd.trainer import OneTransTrainer
    cfg = workload_config('C2')
    cfg.hidden_dim, cfg.num_layers, cfg.ffn_dim, cfg.num_ns_tokens = 128, 2, 256, 4
    cfg.sparse_features = {k: 50 for k in cfg.sparse_features}
    cfg.seq_item_vocab = 200
    cfg._seq_lens = [6, 5, 7]
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    batch = make_batch(32, cfg, seed=1000)
    calls = []
    real = K.ffn_fused_fwd
    monkeypatch.setattr(K, 'ffn_fused_fwd', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])

    def loss(on):
        K.ffn_fused(on)
        del calls[:]
        tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=str(dev), init=P))
        out = tr.train_step(batch)
        torch.cuda.synchronize()
        return out['total_loss'].item(), len(calls)
    l0, n0 = loss(0)
    l0b, _ = loss(0)
    l1, n1 = loss(1)
    print(f'switch: loss off {l0:.7f} / {l0b:.7f}, on {l1:.7f} ({n1} fused calls)')
    assert n0 == 0 and l0 == l0b
    assert n1 >= cfg.num_layers
    assert abs(l1 - l0) <= 2e-5 * max(1.0, abs(l0))
