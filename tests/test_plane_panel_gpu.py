"""The panel form of the pair plane GEMM (gemm_plane.hip plane_panel_kernel: one workgroup per row tile walks its column
tiles, the next tile's first stages copied during the epilogue) and the row metadata parked in LDS (ot_plane_rowmeta)
against the one-tile kernel / the row-map reads on the same operands: every comparison is bit for bit (int32 views, so
NaN fill patterns count).  Ragged row maps (M = 777 over 3 groups: partial tiles, -1 rows), outputs pre-filled with NaN
and five rows longer than the map reaches, so a store to a row that must stay unstored shows.  K = 16 is one k-step
(fewer than the two stages copied ahead), K = 256 more than the C2 model's; N = 384 is read from column tile 1 of a
three-tile image; widths 2, 3 (a one-tile last panel at N = 512) and 4 (the whole row), on the three kernel variants
(three / four workgroups per CU, A's fragments held at K = 128).  ot_plane_panel_launches tells which kernel a launch
took: a forced width runs the panel kernel, auto (1) keeps launches this small on the one-tile kernel."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd._lib import (OT_AX_NONE, OT_AX_RMSNORM, OT_EPI_BIAS, OT_EPI_DROPOUT, OT_EPI_GELU_BWD,
                                OT_EPI_RESIDUAL, OT_EPI_ROW_RSTD, OT_EPI_ROWDOT, OT_GEMM_NT)
from recommend_amd.layout import IMAGE_UNIT_ELEMS, build_map

M, G, PAD = 777, 3, 5
# (image N, first image tile, columns of the GEMM)
SHAPES = [(256, 0, 256), (512, 0, 512), (384, 1, 256)]
KS = [16, 64, 128, 256]


@pytest.fixture(autouse=True)
def split_mode_and_switches(dev):
    old = K.set_matmul_mode('split')
    prev = (K.plane_panel(-1), K.plane_rowmeta(-1))
    yield
    K.plane_panel(prev[0])
    K.plane_rowmeta(prev[1])
    K.set_matmul_mode(old)


def pair_image(W, dev, gamma=None):
    """W [G, N, K] (B[g][n][k]) -> (image, tiles per group) in the pair form (gamma folded, or plain: -2)."""
    G_, N, K_ = W.shape
    base = torch.cat([W.reshape(-1), gamma if gamma is not None else torch.zeros(0)]).float().to(dev)
    desc = torch.tensor([0, K_, 1, N * K_, G_ * N * K_ if gamma is not None else -2, 0, 0, G_, N, K_],
                        dtype=torch.int64, device=dev)
    units = G_ * (N // 128) * (K_ // 16)
    img = torch.zeros(units * IMAGE_UNIT_ELEMS, dtype=torch.int16, device=dev)
    K.split_images(base, desc, 1, units, img)
    return img, N // 128


def ragged_map(rng, M_, G_):
    """Rows of M_ split over G_ groups (uneven counts, so every group has a partial tile)."""
    cuts = np.sort(rng.choice(np.arange(1, M_), G_ - 1, replace=False))
    counts = np.diff(np.concatenate([[0], cuts, [M_]]))
    src, dst = rng.permutation(M_), rng.permutation(M_)
    per, o = [], 0
    for c in counts:
        per.append([src[o:o + c], dst[o:o + c]])
        o += c
    return build_map(per)


_OPS = {}


def operands(dev, K_, N, tn0, ncols):
    """Seeded operands of one shape, built once and shared by every form (never written by a test)."""
    key = (K_, N, tn0, ncols)
    if key not in _OPS:
        rng = np.random.default_rng(1000 * K_ + N + tn0)
        gen = torch.Generator().manual_seed(K_ + N + tn0)
        rm = ragged_map(rng, M, G)
        A = torch.randn(M, K_, generator=gen)
        A *= 10.0 ** (-3 * torch.rand(M, 1, generator=gen))          # rows of different magnitude: different scales
        W = torch.randn(G, N, K_, generator=gen) / math.sqrt(K_)
        gamma = 1 + 0.1 * torch.randn(K_, generator=gen)
        o = dict(rm=rm, d=rm.to(dev), A=A.to(dev), W=W.to(dev), gamma=gamma.to(dev),
                 rstd=torch.rsqrt((A * A).mean(1) + 1e-6).to(dev),
                 bias=(torch.randn(G, ncols, generator=gen) - 0.5).to(dev),
                 aux=torch.randn(M + PAD, ncols, generator=gen).to(dev),
                 amax_a=A.abs().amax(1, keepdim=True).contiguous().to(dev))
        o['img_g'], o['ntn'] = pair_image(W, dev, gamma)
        o['img'], _ = pair_image(W, dev)
        _OPS[key] = o
    return _OPS[key]


def nan(dev, *shape):
    return torch.full(shape, float('nan'), device=dev)


def run_form(dev, form, K_, N, tn0, ncols):
    """One launch of `form` under the current switches; returns its outputs (C first)."""
    o = operands(dev, K_, N, tn0, ncols)
    rm, d, nt = o['rm'], o['d'], ncols // 128
    C = nan(dev, M + PAD, ncols)
    amax = torch.zeros(1, device=dev)
    common = dict(device=dev, amax_out=amax)
    wofs = (o['W'], tn0 * 128 * K_)
    if form in ('rms', 'rms_bias'):
        kw = dict(a_xform=OT_AX_RMSNORM, rstd=o['rstd'], gamma=o['gamma'], bimg=(o['img_g'], o['ntn'], tn0), **common)
        if form == 'rms':
            outs = [C, amax]
            kw['epi'] = 0
        else:
            rmax = nan(dev, M + PAD, nt)
            outs = [C, rmax, amax]
            kw.update(epi=OT_EPI_BIAS, bias=o['bias'], bias_gstride=ncols, rowmax_out=rmax, rowmax_n=nt)
    else:
        rabs = nan(dev, M + PAD, nt)
        kw = dict(a_xform=OT_AX_NONE, a_rowmax=o['amax_a'], a_rowmax_n=1, aux=o['aux'], ldaux=ncols,
                  rowabs_out=rabs, rowabs_n=nt, bimg=(o['img'], o['ntn'], tn0), **common)
        if form == 'gelu_bwd':
            outs = [C, rabs, amax]
            kw['epi'] = OT_EPI_GELU_BWD
        else:
            rdot = nan(dev, M + PAD, nt)
            outs = [C, rabs, rdot, amax]
            kw.update(epi=OT_EPI_GELU_BWD | OT_EPI_ROWDOT, bias=o['bias'], bias_gstride=ncols, rowdot=rdot, rowdot_n=nt)
    K.gemm_rms(OT_GEMM_NT, o['A'], K_, K_, d['rows'][0], wofs, N * K_, K_, ncols, d['tile_group'], rm.ntiles,
               C, ncols, d['rows'][1], **kw)
    torch.cuda.synchronize()
    return outs


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_pair(old, new):
    assert len(old) == len(new)
    C = old[0]
    assert not torch.isnan(C[:M]).any() and torch.isnan(C[M:]).all()      # every mapped row stored, no other
    for a, b in zip(old, new):
        assert same_bits(a, b)
    assert old[-1].item() > 0                                              # amax_out was taken


def run_switch(dev, sw, panel, *args):
    """run_form under ot_plane_panel(sw); `panel`: whether the launch must have taken the panel kernel."""
    K.plane_panel(sw)
    n0 = K.plane_panel_launches()
    outs = run_form(dev, *args)
    assert K.plane_panel_launches() - n0 == (1 if panel else 0)
    return outs


@pytest.mark.parametrize('form', ['rms', 'rms_bias', 'gelu_bwd', 'gelu_bwd_rowdot'])
@pytest.mark.parametrize('N,tn0,ncols', SHAPES)
@pytest.mark.parametrize('K_', KS)
@pytest.mark.parametrize('sw', [1, 2, 102])
def test_panel_bit_identical(dev, sw, K_, N, tn0, ncols, form):
    """Switch 0 against switch 1 (auto: a launch of a few row tiles stays on the one-tile kernel), 2 and 102 (two
    column tiles per workgroup at three / four workgroups per CU), every form the panel kernel has: C, the row maxima /
    bounds / row dots and the tensor bound, bit for bit."""
    old = run_switch(dev, 0, False, form, K_, N, tn0, ncols)
    new = run_switch(dev, sw, sw != 1, form, K_, N, tn0, ncols)
    check_pair(old, new)


@pytest.mark.parametrize('form', ['rms_bias', 'gelu_bwd_rowdot'])
@pytest.mark.parametrize('width', [3, 4, 103, 104, 202, 203, 204])
@pytest.mark.parametrize('K_', [16, 128])
def test_panel_widths_bit_identical(dev, K_, width, form):
    """N = 512 with three column tiles per workgroup (the last panel holds one tile) and with all four, on each
    variant (200 + w holds A's fragments at K = 128 and is the default variant at K = 16)."""
    old = run_switch(dev, 0, False, form, K_, 512, 0, 512)
    new = run_switch(dev, width, True, form, K_, 512, 0, 512)
    check_pair(old, new)


def run_one_tile(dev, form, K_):
    """N = 128 launches (one column tile): the RMSNorm + bias form, and plain A with a residual, dropout and the next
    norm's rstd (the Wo form on the pair)."""
    o = operands(dev, K_, 256, 0, 256)
    rm, d = o['rm'], o['d']
    C = nan(dev, M + PAD, 128)
    if form == 'rms_bias':
        rmax = nan(dev, M + PAD, 1)
        K.gemm_rms(OT_GEMM_NT, o['A'], K_, K_, d['rows'][0], o['W'], 256 * K_, K_, 128, d['tile_group'], rm.ntiles, C,
                   128, d['rows'][1], a_xform=OT_AX_RMSNORM, rstd=o['rstd'], gamma=o['gamma'], epi=OT_EPI_BIAS,
                   bias=o['bias'], bias_gstride=256, rowmax_out=rmax, rowmax_n=1, bimg=(o['img_g'], o['ntn'], 0),
                   device=dev)
        outs = [C, rmax]
    else:
        rs = nan(dev, M + PAD)
        K.gemm_rms(OT_GEMM_NT, o['A'], K_, K_, d['rows'][0], o['W'], 256 * K_, K_, 128, d['tile_group'], rm.ntiles, C,
                   128, d['rows'][1], a_xform=OT_AX_NONE, a_rowmax=o['amax_a'], a_rowmax_n=1,
                   epi=OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD, res=o['aux'], ldres=256, res_tok=0, seed=17,
                   site=2, drop=0.2, tail=(1, 1), rstd_out=rs, eps=1e-6, bimg=(o['img'], o['ntn'], 0), device=dev)
        outs = [C, rs]
    torch.cuda.synchronize()
    return outs


def test_panel_leaves_one_tile_launch(dev):
    """ntn == 1: the switch does not apply (the launch stays on plane_gemm_kernel; the host picks the panel form only
    for two or more column tiles) — the outputs are the same bits with it on, off or forced wide."""
    outs = []
    n0 = K.plane_panel_launches()
    for sw in (0, 1, 4, 104, 204):
        K.plane_panel(sw)
        outs.append(run_one_tile(dev, 'rms_bias', 128))
    assert K.plane_panel_launches() == n0                   # no launch took the panel kernel
    assert not torch.isnan(outs[0][0][:M]).any() and torch.isnan(outs[0][0][M:]).all()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert same_bits(a, b)


@pytest.mark.parametrize('form', ['rms_bias', 'res_drop_rstd'])
@pytest.mark.parametrize('K_', [16, 128])
def test_rowmeta_bit_identical(dev, K_, form):
    """The one-tile kernel alone (panel off): row metadata read from the row maps (0) against parked in LDS (1), on
    a row-scale (RMSNorm prologue) launch and a residual + dropout + rstd launch; and on the N = 512 row-scale
    launch, where each row tile's metadata is loaded by four workgroups."""
    K.plane_panel(0)
    res = []
    for sw in (0, 1):
        K.plane_rowmeta(sw)
        r = run_one_tile(dev, form, K_)
        if form == 'rms_bias':
            r += run_form(dev, 'rms_bias', K_, 512, 0, 512)
        res.append(r)
    C = res[0][0]
    assert not torch.isnan(C[:M]).any() and torch.isnan(C[M:]).all()
    for a, b in zip(res[0], res[1]):
        assert same_bits(a, b)
