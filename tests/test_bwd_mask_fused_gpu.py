"""The FFN dropout's backward inside the fused FFN backward and the W2 weight gradient (ot_ffn_fused_bwd_mask,
ot_mixed_gemm_wgrad_keep / OT_WG_D_KEEPBITS; switch ONETRANS_BWD_MASK_FUSED): no dropout pass, dY2 never exists.

Kernel level, at 185 rows (a ragged second tile) and 128 rows, d 128, f 128 / 512, one and three weight groups (row
maps with -1 rows), rate 0.1, tail maps Kq == I and Kq < I (I 37, Kq 5: tail_token):

1. keep_out equals oracle/keras_math.py::dropout_keep for every named row and column; rows no map names stay unwritten.
2. Given row bounds b with f32(b x scale) in the binade of the dropout pass's row maxima (the kernel reads only the
   exponent of scale x bound: common.h pow2_scale14), du, max |du|, dx1, dyo, dgamma, the rowabs parts and the dyo amax
   equal {ot_dropout_apply_ex, ot_ffn_fused_bwd on its dy2} bit for bit.
3. dW2 and db2 of the keep-bits weight gradient equal the weight gradient on the materialised dy2 whose d_bound is
   f32(scale x the keep-bits call's d_bound), bit for bit.
4. With the row bounds of the unmasked dx2 (what the model passes): max |error| against float64 at most 4 x the native
   f32 path's (+ 8 ulp of the scale) on the normal, outlier and zero_rows operand sets of test_ffn_fused_bwd_gpu.py.
   Measured ratios (mask mode / f32): du 0.51 - 0.69, dx1 0.52 - 0.73; every figure is in profiles/r15/bwd_mask_fused.md.

Model level (2 layers, d 128, B 37, dropout 0.1; plain / accumulate / recompute): every gradient bank within 4 x the
switched-off path's error against the float64 oracle + 8 ulp; two runs bit-identical; with the gate true no
dropout_apply launch (a rows_absmax launch stands in for it exactly in the blocks whose dx2 has no producer bounds);
with the gate false the launch list and every output bit are the switched-off model's."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle.keras_math import dropout_keep
from recommend_amd import _lib
from recommend_amd import kernels as K
from recommend_amd._lib import OT_AX_GELU, OT_WG_D_KEEPBITS

import test_ffn_fused_bwd_gpu as T

gpu = pytest.mark.gpu

D, PAD = T.D, T.PAD
RATE = 0.1
SCALE = np.float32(1.0) / (np.float32(1.0) - np.float32(RATE))       # the library's f32 1 / (1 - p)
SEED, SITE, MASK_SITE = 1234, 2, 3
SENTINEL = 0x5A5A5A5A
NEW_VS_OLD = 4.0
# (rows, f, groups, (Kq, I))
SHAPES = [(185, 512, 3, (5, 37)), (185, 128, 1, (37, 37)), (128, 128, 3, (5, 37)), (128, 512, 1, (37, 37))]


@pytest.fixture
def switches(dev):
    old = K.set_matmul_mode('split')
    prev = K.ffn_fused_bwd_on(-1), K.bwd_mask_fused(-1), K.last_fold(-1)
    yield
    K.ffn_fused_bwd_on(prev[0])
    K.bwd_mask_fused(prev[1])
    K.last_fold(prev[2])
    K.set_probe(None)
    K.set_matmul_mode(old)


_OPS = {}


def operands(dev, shape, case='normal'):
    """Seeded operands of one shape (never written by a test); o['dy2'] holds dx2, the gradient before the mask, and
    o['rmax'] its rows' maxima; with ``case`` normal the residual gradient is dx2 itself, as in the block backward."""
    key = (shape, case)
    if key not in _OPS:
        M, f, G, _ = shape
        rng = np.random.default_rng(13 * f + G + M)
        gen = torch.Generator().manual_seed(f + G + M + len(case))
        dx2 = torch.randn(M, D, generator=gen) * 10.0 ** (-2 * torch.rand(M, 1, generator=gen))
        if case == 'outlier':
            dx2[torch.arange(M), torch.randint(0, D, (M,), generator=gen)] *= 1e4
        elif case == 'zero_rows':
            dx2[::3] = 0.0
        _OPS[key] = T.device_ops(dev, T.row_map(rng, M, G), dx2, 1.5 * torch.randn(M, f, generator=gen),
                                 torch.randn(M, D, generator=gen), dx2 if case == 'normal' else None,
                                 1 + 0.1 * torch.randn(D, generator=gen),
                                 torch.randn(G, f, D, generator=gen) / math.sqrt(f),
                                 torch.randn(G, D, f, generator=gen) / math.sqrt(D))
    return _OPS[key]


def token_of(rows, tail):
    """common.h tail_token: the layer-input token of compact row r."""
    Kq, I = tail
    b = rows // Kq
    return rows if Kq == I else b * I + (I - Kq) + (rows - b * Kq)


def keep_ref(M, tail, site=MASK_SITE):
    idx = token_of(np.arange(M, dtype=np.int64), tail)[:, None] * D + np.arange(D, dtype=np.int64)[None, :]
    return dropout_keep(SEED, site, idx, RATE)                        # [M, D] bool


def pack_bits(keep, dev, rows):
    """[M, D] bool -> [rows, D / 32] int32, bit c % 32 of word c / 32 (rows past M: zeros)."""
    b = np.packbits(keep.astype(np.uint8), axis=1, bitorder='little').view(np.int32)
    out = torch.zeros(rows, D // 32, dtype=torch.int32, device=dev)
    out[:keep.shape[0]] = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    return out


def run_mask(dev, o, shape, rmax):
    """ot_ffn_fused_bwd_mask on dx2 with the row bounds ``rmax``; returns the outputs and keep_out."""
    M, f, G, tail = shape
    rm, d = o['rm'], o['d']
    r = T.outputs(dev, M, f, RATE)
    keep = torch.full((M + PAD, D // 32), SENTINEL, dtype=torch.int32, device=dev)
    K.ffn_fused_bwd(o['dy2'], D, rmax, 1, d['rows'][1], d['tile_group'], rm.ntiles, o['img2'], G, o['img1'], G, f,
                    o['u'], f, r['du'], f, o['x1'], D, o['gamma'], o['rstd'], r['dx1'], D, r['dg'], du_amax=r['b_du'],
                    dres=o['dres'], lddres=D, dx_masked=r['dyo'], lddxm=D, amax_out=r['b_dyo'], rowabs_out=r['rm_dyo'],
                    rowabs_n=1, seed=SEED, site=SITE, drop=RATE, tail=tail, device=dev, mask_site=MASK_SITE,
                    keep_out=keep, ldkeep=D // 32)
    torch.cuda.synchronize()
    return r, keep


def dropout_pass(dev, o, shape):
    """The pass the mask mode replaces: (dy2, its amax, its row maxima) of ot_dropout_apply_ex."""
    M, _, _, tail = shape
    dy2, amax, rmax = T.nan(dev, M, D), torch.zeros(1, device=dev), T.nan(dev, M, 1)
    K.dropout_apply(o['dy2'], D, dy2, D, M, D, SEED, MASK_SITE, RATE, tail, amax=amax, rowmax=rmax)
    return dy2, amax, rmax


def binade(x):
    return torch.frexp(x)[1]


def bounds_with_scale_of(rm_dy2):
    """Row bounds b with f32(b x SCALE) in rm_dy2's binade (equal to it where the division is exact)."""
    s = torch.tensor(float(SCALE), device=rm_dy2.device)
    b = rm_dy2 / s
    for step in (math.inf, -math.inf):
        bad = binade(b * s) != binade(rm_dy2)
        b = torch.where(bad, torch.nextafter(b, torch.full_like(b, step)), b)
    assert torch.equal(binade(b * s), binade(rm_dy2))
    return b


# ------------------------------------------------------------------------------------------------ kernel level
@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'M{s[0]}-f{s[1]}-G{s[2]}-K{s[3][0]}')
def test_keep_bits_and_bit_identity(dev, switches, shape):
    M, f, G, tail = shape
    o = operands(dev, shape)
    dy2, _, rm_dy2 = dropout_pass(dev, o, shape)
    a, keep = run_mask(dev, o, shape, bounds_with_scale_of(rm_dy2))
    # 1. the keep bits
    want = keep_ref(M, tail)
    assert 0.05 < 1.0 - want.mean() < 0.15
    assert torch.equal(keep[:M], pack_bits(want, dev, M)), 'keep_out differs from dropout_keep'
    assert (keep[M:] == SENTINEL).all(), 'keep_out written for rows no map names'
    assert torch.equal(dy2 != 0, torch.from_numpy(want).to(dev) & (o['dy2'] != 0))
    # 2. bit identity with {dropout pass, fused backward on dy2}
    b = T.run_fused(dev, dict(o, dy2=dy2, rmax=rm_dy2), f, G, RATE, tail=tail, seed=SEED, site=SITE)
    assert b['b_du'].item() > 0 and not torch.isnan(a['du'][:M]).any() and torch.isnan(a['du'][M:]).all()
    for k in ('du', 'b_du', 'dx1', 'dyo', 'dg', 'rm_dyo', 'b_dyo'):
        assert T.same_bits(a[k], b[k]), f'{k} differs from the dropout pass + ot_ffn_fused_bwd'
    again, keep2 = run_mask(dev, o, shape, bounds_with_scale_of(rm_dy2))
    assert torch.equal(keep, keep2) and all(T.same_bits(a[k], again[k]) for k in ('du', 'dx1', 'dyo', 'dg'))


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'M{s[0]}-f{s[1]}-G{s[2]}-K{s[3][0]}')
def test_weight_gradient_from_keep_bits(dev, switches, shape):
    M, f, G, tail = shape
    o = operands(dev, shape)
    rm, d = o['rm'], o['d']
    dy2, _, _ = dropout_pass(dev, o, shape)
    keep = pack_bits(keep_ref(M, tail), dev, M)
    a_bound = o['u'].abs().max().reshape(1)
    bk = o['dy2'].abs().max().reshape(1)                              # of dx2: the kernel multiplies it by the scale
    bd = bk * torch.tensor(float(SCALE), device=dev)                   # the same f32 product, for the materialised dy2
    out = []
    for D_, kw, ax in ((dy2, dict(d_bound=bd), OT_AX_GELU),
                       (o['dy2'], dict(d_bound=bk, keep=keep, ldkeep=D // 32, d_scale=float(SCALE)),
                        OT_AX_GELU | OT_WG_D_KEEPBITS)):
        dW, db = T.nan(dev, G, f, D), T.nan(dev, G, D)
        K.wgrad(o['u'], f, d['rows'][1], D_, D, d['rows'][1], f, D, d, rm.chunks.shape[0], G, dW, f * D, db, D,
                a_xform=ax, device=dev, a_bound=a_bound, **kw)
        torch.cuda.synchronize()
        out.append((dW, db))
    (w0, b0), (w1, b1) = out
    assert torch.isfinite(w0).all() and w0.abs().max().item() > 0 and b0.abs().max().item() > 0
    assert T.same_bits(w1, w0), 'dW2 differs from the weight gradient on the materialised dy2'
    assert T.same_bits(b1, b0), 'db2 differs from the weight gradient on the materialised dy2'
    ref = torch.einsum('mf,md->mfd', torch.nn.functional.gelu(o['u'].double()), dy2.double())
    g = T.group_of_row(rm, M).to(dev)
    want = torch.stack([ref[g == i].sum(0) for i in range(G)])
    assert (w1.double() - want).abs().max().item() <= 1e-5 * max(want.abs().max().item(), 1.0)


@gpu
@pytest.mark.parametrize('case', ['normal', 'outlier', 'zero_rows'])
def test_precision_bar_with_producer_bounds(dev, switches, case):
    """Row bounds of the unmasked dx2 (the model's: its producer's rowabs_out, or ot_rows_absmax), against float64 beside
    the native f32 launches on the materialised dy2; no residual gradient, as in test_ffn_fused_bwd_gpu.py."""
    shape = (185, 512, 3, (5, 37))
    M, f, G, tail = shape
    o = operands(dev, shape, case if case != 'normal' else 'plain')
    g = T.group_of_row(o['rm'], M)
    dy2, _, _ = dropout_pass(dev, o, shape)
    a, _ = run_mask(dev, o, shape, o['rmax'])
    old = K.set_matmul_mode('f32')
    try:
        b = T.run_unfused(dev, dict(o, dy2=dy2), f, G, RATE, tail, seed=SEED, site=SITE, images=False)
    finally:
        K.set_matmul_mode(old)
    c = lambda t: t.double().cpu()
    r, x1 = c(o['rstd'])[:, None], c(o['x1'])
    dU = torch.einsum('mk,mfk->mf', c(dy2), c(o['W2'])[g]) * T.gelu_grad64(c(o['u']))
    gv = torch.einsum('mf,mnf->mn', dU, c(o['W1'])[g]) * c(o['gamma'])
    ref = gv * r - x1 * (r ** 3 * (gv * x1).sum(1, keepdim=True) / D)
    assert torch.isfinite(a['dx1'][:M]).all() and torch.isfinite(a['du'][:M]).all()
    if case == 'zero_rows':
        assert (a['du'][:M][::3] == 0).all() and (a['dx1'][:M][::3] == 0).all()
    for k, want in (('du', dU), ('dx1', ref)):
        e_pair = (c(a[k][:M]) - want).abs().max().item()
        e_f32 = (c(b[k][:M]) - want).abs().max().item()
        scale = want.abs().max().item()
        floor = 8 * 2.0 ** -24 * scale
        print(f'bwd_mask_fused {case} {k}: pair {e_pair:.3e}  f32 {e_f32:.3e}  '
              f'ratio {e_pair / max(e_f32, 1e-300):.2f}  (scale {scale:.2e})')
        assert e_pair <= NEW_VS_OLD * e_f32 + floor, f'{case} {k}: mask mode {e_pair:.3e} > {NEW_VS_OLD} x f32 {e_f32:.3e}'


# ------------------------------------------------------------------------------------------------ model level
def run_model(cfg, dev, P, batch, mask, fused=True, accumulate=False, fuse_bwd=None):
    K.bwd_mask_fused(int(mask))
    return T.run_model(cfg, dev, P, batch, fused, accumulate, fuse_bwd)


def count(labels, what):
    return sum(what in s for s in labels)


@gpu
@pytest.mark.parametrize('variant,fold', [('plain', 0), ('accumulate', 0), ('recompute', 0), ('plain', 1)])
def test_model_precision_bar(dev, switches, variant, fold):
    """``fold`` 0: the last block runs the QKV dgrad, whose epilogue reports the bounds of block 0's dx2 (no pass over
    it at all); 1: it takes the folded attention, and block 0's bounds come from the row-absmax pass, like block 1's."""
    from recommend_amd.data import make_batch
    from recommend_amd.params import init_params
    K.last_fold(fold)
    cfg = T.model_cfg(dropout=RATE, recompute_blocks=variant == 'recompute')
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    batch = make_batch(T.B_MODEL, cfg, seed=1000)
    acc = variant == 'accumulate'
    p1, g1, seed, lab1 = run_model(cfg, dev, P, batch, True, accumulate=acc)
    p1b, g1b, _, lab1b = run_model(cfg, dev, P, batch, True, accumulate=acc)
    p0, g0, seed0, lab0 = run_model(cfg, dev, P, batch, False, accumulate=acc)
    assert seed == seed0 and lab1 == lab1b
    # the forward is untouched; the backward's dropout passes are gone, a row-absmax pass in the blocks without
    # producer bounds (the last block always: its dx2 comes from the head)
    assert same_forward(lab1, lab0) and T.same_bits(p1, p0)
    assert count(lab0, 'dropout_apply') == cfg.num_layers and count(lab1, 'dropout_apply') == 0
    assert count(lab1, 'rows_absmax') - count(lab0, 'rows_absmax') == (2 if fold else 1)
    assert count(lab1, 'ffn_fused_bwd') == count(lab0, 'ffn_fused_bwd') == cfg.num_layers
    assert T.same_bits(p1, p1b), 'probs differ between two runs'
    for n in g1:
        assert T.same_bits(g1[n], g1b[n]), f'{n}: two runs differ'
    rp, rg = T.oracle(cfg, (RATE,), P, batch, seed)
    e1 = T.errors(p1, g1, rp, rg, 1.0 if acc else 0.0)
    e0 = T.errors(p0, g0, rp, rg, 1.0 if acc else 0.0)
    for n in e1:
        (a, scale), (b, _) = e1[n], e0[n]
        floor = 8 * 2.0 ** -24 * max(scale, 1.0 if acc else 0.0)
        print(f'fold{fold} {variant} {n}: mask fused {a:.3e}  old {b:.3e}  ratio {a / max(b, 1e-300):.2f}  '
              f'(scale {scale:.2e})')
        assert math.isfinite(a)
        assert a <= NEW_VS_OLD * b + floor, f'{n}: mask-fused error {a:.3e} > {NEW_VS_OLD} x old {b:.3e}'


def same_forward(lab1, lab0):
    """The launch lists agree up to the backward's first launch (the head's backward follows the forward)."""
    n = next(i for i, (x, y) in enumerate(zip(lab1, lab0)) if x != y)
    return n > 0 and not any('dropout_apply' in s for s in lab0[:n])


GATE_CASES = dict(T.GATE_CASES, dropout0=dict(cfg=dict(dropout=0.0)), ffn_fused_bwd_off=dict(fused=False),
                  padding_mask=dict(cfg=dict(seq_padding_mask=True)))


@gpu
@pytest.mark.parametrize('name', list(GATE_CASES))
def test_gate_false_runs_the_old_launches(dev, switches, monkeypatch, name):
    from recommend_amd.data import make_batch
    from recommend_amd.params import init_params
    case = GATE_CASES[name]
    for k, v in case.get('env', {}).items():
        monkeypatch.setenv(k, v)
    cfg = T.model_cfg(**{'dropout': RATE, **case.get('cfg', {})})
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    ns, seq, lab = make_batch(T.B_MODEL, cfg, seed=1000)
    if name == 'padding_mask':
        import test_last_fold_gpu as LF
        seq = {**seq, **LF.ragged_lengths(T.B_MODEL, cfg, seed=11)}
    kw = dict(fused=case.get('fused', True), fuse_bwd=case.get('fuse_bwd'))
    p1, g1, _, lab1 = run_model(cfg, dev, P, (ns, seq, lab), True, **kw)
    p0, g0, _, lab0 = run_model(cfg, dev, P, (ns, seq, lab), False, **kw)
    assert lab1 == lab0 and len(lab1) > 0
    assert count(lab1, 'dropout_apply') == (cfg.num_layers if cfg.dropout_rate > 0 else 0)
    assert T.same_bits(p1, p0)
    for n in g1:
        assert T.same_bits(g1[n], g0[n]), n


@gpu
def test_switch_off_is_the_parent_path(dev, switches):
    """Inside the gate with the switch off: the dropout pass per block, no keep-bits launch, two runs bit-identical."""
    from recommend_amd.data import make_batch
    from recommend_amd.params import init_params
    cfg = T.model_cfg(dropout=RATE)
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    batch = make_batch(T.B_MODEL, cfg, seed=1000)
    p0, g0, _, lab0 = run_model(cfg, dev, P, batch, False)
    p0b, g0b, _, lab0b = run_model(cfg, dev, P, batch, False)
    assert lab0 == lab0b and count(lab0, 'dropout_apply') == cfg.num_layers
    assert T.same_bits(p0, p0b)
    for n in g0:
        assert T.same_bits(g0[n], g0b[n]), n


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')
def test_bad_arguments_are_refused():
    a = T.bwd_args(drop_rate=0.1, tail_K=1, tail_I=1, dx_masked=4096, lddxm=128)
    with pytest.raises(_lib.OneTransHipError, match='keep_out'):
        _lib.call('ot_ffn_fused_bwd_mask', ctypes.byref(a), 3, None, 4, None)
    with pytest.raises(_lib.OneTransHipError, match='keep_out'):
        _lib.call('ot_ffn_fused_bwd_mask', ctypes.byref(a), 3, 4096, 2, None)          # ldkeep < 4
    with pytest.raises(_lib.OneTransHipError, match='drop_rate > 0'):
        _lib.call('ot_ffn_fused_bwd_mask', ctypes.byref(T.bwd_args()), 3, 4096, 4, None)
    with pytest.raises(_lib.OneTransHipError, match='OT_WG_D_KEEPBITS'):
        _lib.call('ot_mixed_gemm_wgrad_keep', 4096, 128, None, OT_AX_GELU, 4096, 128, None, 128, 128, 4096, 1, 4096, 1,
                  4096, 128 * 128, None, 0, 0, 4096, 1 << 20, 4096, 4096, 4096, 4, 1.0, 1, None)
    with pytest.raises(_lib.OneTransHipError, match='OT_WG_D_KEEPBITS needs'):             # f32 mode: no pair form
        _lib.call('ot_mixed_gemm_wgrad_keep', 4096, 128, None, OT_AX_GELU | OT_WG_D_KEEPBITS, 4096, 128, None, 128, 128,
                  4096, 1, 4096, 1, 4096, 128 * 128, None, 0, 0, 4096, 1 << 20, 4096, 4096, 4096, 4, 1.0, 0, None)
    assert _lib.size('ot_bwd_mask_fused', -1) in (0, 1)
