"""GPU: every attention route against float64 on saturating and peaked softmax rows (tests/attn_edges_ref.py: the
cases, the reference, the yardsticks; tests/test_attn_edges_ref.py proves the cases discriminating on the CPU).

Each output (out, lse, dq, dk, dv — and the cached rows' dk, dv) is pre-filled with NaN or the sentinel, must come
back finite, and must satisfy

    max |kernel - float64|  <=  MARGIN * yardstick + 8 * 2^-24 * max |float64|

The yardstick is the error of the same operation evaluated in float32 on the CPU; for the gradients of the
f32-arithmetic backwards (wave, FDL, short tail, cached, masked) the larger of that and of the recomputing algorithm's
float32 evaluation (attn_edges_ref.evaluate_recompute says why); in bf16 mode the error of the float64 evaluation with
the bf16 kernels' roundings.  The margins were fixed before the first GPU run (attn_edges_ref.MARGIN_*);
profiles/r19/attn_softmax_edges.md has the reasoning and the measured table.  A route is asserted with the library's
own queries where one exists; every 'EDGE ...' line printed here is a row of that table.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_edges_ref as AE
from recommend_amd import _lib
from recommend_amd import kernels as K

SENTINEL = 12345.0


def check(tag, ref, yards, outputs, margin):
    """outputs {name: (kernel tensor, pick)}; pick(evaluation) -> that output.  The yardstick of an output is the
    largest error among the evaluations ``yards``.  Prints one table row per output, then asserts them all."""
    bad = []
    for name, (got, pick) in outputs.items():
        want = pick(ref)
        e_yard = max(AE.err(pick(y), want) for y in yards)
        finite = bool(torch.isfinite(got).all())
        e = AE.err(got, want) if finite else float('inf')
        b = AE.bound(e_yard, want, margin)
        print(f'EDGE {tag} {name} yard {e_yard:.3e} kernel {e:.3e} ratio {e / max(e_yard, 1e-300):.2f} '
              f'margin {margin} bound {b:.3e} scale {want.abs().max().item():.2e}')
        if not finite:
            bad.append(f'{name}: not finite')
        elif e > b:
            bad.append(f'{name}: {e:.3e} > {margin} x {e_yard:.3e} + floor = {b:.3e}')
    assert not bad, bad


def fwd_outputs(out, lse):
    return {'out': (out, lambda r: r['out']), 'lse': (lse, lambda r: r['lse'])}


def grad_outputs(g, d, leaf=0, names=('dq', 'dk', 'dv'), first=0, rows=lambda t: t):
    """Column blocks first, first + 1, .. of width d of gradient ``leaf``, named; ``rows`` restricts the rows."""
    return {name: (rows(g)[..., (first + i) * d:(first + i + 1) * d],
                   lambda r, i=i: rows(r['grads'][leaf])[..., (first + i) * d:(first + i + 1) * d])
            for i, name in enumerate(names)}


# ------------------------------------------------------------------------------------------------ routes
def assert_fwd_route(route, mode, shape, sel):
    B, H, I, Kq, hd = shape
    lib, prec = _lib.load(), _lib.MATMUL_MODES[mode]
    slice_fwd = bool(lib.ot_attn_amax_supported(I, Kq, hd, int(sel), prec) & 1)      # the slice forward reports max |O|
    assert slice_fwd == (route == 'SLICE'), (route, mode, shape)
    if route == 'SLICE' and not sel:
        assert lib.ot_attn_slice_supported(I, Kq, hd, 0)


def assert_bwd_route(route, mode, shape, sel):
    B, H, I, Kq, hd = shape
    lib, prec = _lib.load(), _lib.MATMUL_MODES[mode]
    base = K.size('ot_attn_bwd_workspace_size', B, H, Kq)
    kgroup = bool(lib.ot_attn_bwd_dqkv_bf16_supported(I, Kq, hd, int(sel), prec))
    assert kgroup == (route == 'KGROUP'), (route, mode, shape)
    if kgroup:
        assert K.size('ot_attn_bwd_ex_workspace_size', B, H, I, Kq, hd, int(sel), prec) > base
    # the backward reports max |dQKV| on the slice route (the short tail reports it too, so TAIL entries are not asked)
    if route != 'TAIL':
        assert bool(lib.ot_attn_amax_supported(I, Kq, hd, int(sel), prec) & 2) == (route == 'SLICE'), (route, mode, shape)
    # FDL, WAVE, TAIL and BF16 (and TAIL, SHARED_KV, WAVE, PLANES in the forward) have no query of their own: there
    # the route name is the one the existing tests argue for the shape, a label, beyond "not SLICE, not KGROUP"


# ------------------------------------------------------------------------------------------------ plain layouts
@functools.lru_cache(maxsize=None)
def run_plain(dev, mode, shape, sel, case, masked=False):
    """Forward and backward of one problem through the library; the backward takes the kernel's own O and lse, as a
    model does.  Returns CPU float64 (out, lse [B, H, Kq], dqkv)."""
    B, H, I, Kq, hd = shape
    d = H * hd
    p = AE.plain_problem(case, B, H, I, Kq, hd, sel, masked, operands_bf16=mode == 'bf16')
    qkv_d, dout_d = p['qkv'].float().to(dev), p['dout'].float().to(dev)
    qp_d = p['qpos'].to(torch.int32).reshape(-1).to(dev) if sel else None
    out = torch.full((B * Kq, d), float('nan'), device=dev)
    lse = torch.full((B * H * Kq,), float('nan'), device=dev)
    dqkv = torch.full((B * I, 3 * d), float('nan'), device=dev)
    if Kq < I:
        dqkv[:, :d].zero_()                                             # dQ only on the query rows
    with K.precision(mode):
        if masked:
            wide = torch.zeros(B, I + 5, dtype=torch.uint8)             # a layer's slice of a wider array
            wide[:, 5:] = p['valid'].to(torch.uint8)
            kv = (wide.to(dev), 5, I + 5)
            K.attn_fwd_masked(qkv_d, 3 * d, B, H, I, Kq, hd, out, lse, kv, qpos=qp_d)
            K.attn_bwd_masked(qkv_d, 3 * d, out, dout_d, lse, B, H, I, Kq, hd, dqkv, kv, qpos=qp_d)
        else:
            K.attn_fwd(qkv_d, 3 * d, B, H, I, Kq, hd, out, lse, qpos=qp_d)
            K.attn_bwd(qkv_d, 3 * d, out, dout_d, lse, B, H, I, Kq, hd, dqkv, qpos=qp_d)
    torch.cuda.synchronize()
    return out.double().cpu(), lse.double().cpu().reshape(B, H, Kq), dqkv.double().cpu()


@functools.lru_cache(maxsize=None)
def bf16_yardstick(shape, sel, case, planes_bwd):
    B, H, I, Kq, hd = shape
    assert hd >= 32                                                     # the one-plane forward
    p = AE.plain_problem(case, B, H, I, Kq, hd, sel, operands_bf16=True)
    return AE.bf16_emulation(p['qkv'], p['dout'], B, H, I, hd, p['qpos'], planes_fwd=True, planes_bwd=planes_bwd)


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('entry', AE.FWD, ids=map(AE.entry_id, AE.FWD))
def test_forward(dev, entry, case):
    route, mode, shape, sel = entry
    B, H, I, Kq, hd = shape
    assert_fwd_route(route, mode, shape, sel)
    p = AE.plain_problem(case, B, H, I, Kq, hd, sel, operands_bf16=mode == 'bf16')
    out, lse, _ = run_plain(dev, mode, shape, sel, case)
    if mode == 'bf16':
        yards, margin = [bf16_yardstick(shape, sel, case, True)], AE.MARGIN_BF16
    else:
        yards, margin = [p['f32']], AE.MARGIN_PAIR if route == 'SLICE' and hd == 64 else AE.MARGIN_F32
    check(f'fwd {AE.entry_id(entry)} {case}', p['ref'], yards, fwd_outputs(out, lse), margin)


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('entry', AE.BWD, ids=map(AE.entry_id, AE.BWD))
def test_backward(dev, entry, case):
    route, mode, shape, sel = entry
    B, H, I, Kq, hd = shape
    assert_bwd_route(route, mode, shape, sel)
    p = AE.plain_problem(case, B, H, I, Kq, hd, sel, operands_bf16=mode == 'bf16')
    _, _, dqkv = run_plain(dev, mode, shape, sel, case)
    if mode == 'bf16':                  # P / dS rounded where the backward runs on bf16 planes
        yards, margin = [bf16_yardstick(shape, sel, case, route in ('KGROUP', 'BF16'))], AE.MARGIN_BF16
    elif route == 'SLICE':
        yards, margin = [p['f32']], AE.MARGIN_PAIR
    else:
        yards, margin = [p['f32'], p['rec32']], AE.MARGIN_F32
    check(f'bwd {AE.entry_id(entry)} {case}', p['ref'], yards, grad_outputs(dqkv, H * hd), margin)


@pytest.mark.parametrize('case', AE.MASKED_CASES)
@pytest.mark.parametrize('shape', AE.MASKED, ids=lambda s: '-'.join(map(str, s)))
def test_masked(dev, shape, case):
    """ot_attn_fwd_masked / ot_attn_bwd_masked (the short-tail kernels at K <= 4, else the one-wave kernels, in their
    MASK instantiations): 'rising' under a random mask, and the padding keys holding the largest scores."""
    B, H, I, Kq, hd = shape
    p = AE.plain_problem(case, B, H, I, Kq, hd, masked=True)
    out, lse, dqkv = run_plain(dev, 'split', shape, False, case, masked=True)
    tag = f'masked {"TAIL" if Kq <= 4 else "WAVE"}-' + '-'.join(map(str, shape)) + f' {case}'
    check(tag, p['ref'], [p['f32']], fwd_outputs(out, lse), AE.MARGIN_F32)
    check(tag, p['ref'], [p['f32'], p['rec32']], grad_outputs(dqkv, H * hd), AE.MARGIN_F32)


# ------------------------------------------------------------------------------------------------ cached layouts
def _req_dev(p, dev):
    return p['req'].to(torch.int32).to(dev)


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('H,hd,Ic,n,Kq', AE.CACHED)
def test_cached(dev, H, hd, Ic, n, Kq, case):
    """ot_attn_fwd_cached_lse / ot_attn_bwd_cached: the dominant key in the cache ('falling') or in the own rows
    ('rising'); rows wider than the operands, the padding and the rows without a query untouched."""
    p = AE.cached_problem(case, AE.CANDS, H, Ic, n, Kq, hd)
    d, R, C = H * hd, len(AE.CANDS), sum(AE.CANDS)
    ld, ldc = 3 * d + 8, 2 * d + 4
    g = torch.Generator().manual_seed(3)
    qkv_d = torch.cat([p['qkv'].float(), torch.randn(C * n, ld - 3 * d, generator=g)], 1).to(dev)
    kv_d = torch.cat([p['kv'].float(), torch.randn(R * Ic, ldc - 2 * d, generator=g)], 1).to(dev)
    dout_d = p['dout'].float().to(dev)
    req_d = _req_dev(p, dev)
    req_start = torch.searchsorted(req_d, torch.arange(R + 1, device=dev, dtype=torch.int32)).to(torch.int32)
    out = torch.full((C * Kq, d), float('nan'), device=dev)
    lse = torch.full((C, H, Kq), float('nan'), device=dev)
    K.attn_fwd_cached_lse(qkv_d, ld, kv_d, ldc, req_d, C, H, Ic, n, Kq, hd, out, lse)
    dqkv = torch.full((C * n, ld), SENTINEL, device=dev)
    dkv = torch.full((R * Ic, ldc), SENTINEL, device=dev)
    K.attn_bwd_cached(qkv_d, ld, kv_d, ldc, req_start, R, C, H, Ic, n, Kq, hd, out, dout_d, lse, dqkv, dkv)
    torch.cuda.synchronize()
    got, gkv = dqkv.double().cpu(), dkv.double().cpu()
    assert (got.reshape(C, n, ld)[:, :n - Kq, :d] == SENTINEL).all()      # rows without a query: dq not written
    assert (got[:, 3 * d:] == SENTINEL).all() and (gkv[:, 2 * d:] == SENTINEL).all()        # nor the row padding
    tag = f'cached WAVE-{H}-{hd}-Ic{Ic}-n{n}-K{Kq} {case}'
    check(tag, p['ref'], [p['f32']], fwd_outputs(out.double().cpu(), lse.double().cpu()), AE.MARGIN_F32)
    yards = [p['f32'], p['rec32']]
    kept = lambda t: t.reshape(C, n, -1)[:, n - Kq:]
    check(tag, p['ref'], yards, grad_outputs(got, d, names=('dq',), rows=kept), AE.MARGIN_F32)
    check(tag, p['ref'], yards, grad_outputs(got, d, names=('dk', 'dv'), first=1), AE.MARGIN_F32)
    check(tag, p['ref'], yards, grad_outputs(gkv, d, leaf=1, names=('dk_cache', 'dv_cache')), AE.MARGIN_F32)


@pytest.mark.parametrize('case', AE.CASES + ('dominant_invalid',))
def test_cached_masked(dev, case):
    """ot_attn_fwd_cached_masked under a random cache mask; 'dominant_invalid': the masked cached keys hold +120."""
    cands, H, hd, Ic, n, Kq = AE.CACHED_MASKED
    p = AE.cached_problem(case, cands, H, Ic, n, Kq, hd, masked=True)
    d, C = H * hd, sum(cands)
    out = torch.full((C * Kq, d), float('nan'), device=dev)
    lse = torch.full((C, H, Kq), float('nan'), device=dev)
    cv = p['cache_valid'].to(torch.uint8).to(dev)
    K.attn_fwd_cached_masked(p['qkv'].float().to(dev), 3 * d, p['kv'].float().to(dev), 2 * d, _req_dev(p, dev), C, H, Ic,
                             n, Kq, hd, out, (cv, 0, Ic), lse)
    torch.cuda.synchronize()
    check(f'cached_masked H{H}-{hd}-Ic{Ic}-n{n}-K{Kq} {case}', p['ref'], [p['f32']],
          fwd_outputs(out.double().cpu(), lse.double().cpu()), AE.MARGIN_F32)


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('cands,H,hd,Ic,n,Kq', AE.KV16)
def test_cached_kv16(dev, cands, H, hd, Ic, n, Kq, case):
    """ot_attn_fwd_cached_kv16: f32 arithmetic over a bf16 cache; the reference runs on the rounded cache."""
    p = AE.cached_problem(case, cands, H, Ic, n, Kq, hd, cache_bf16=True)
    d, R, C = H * hd, len(cands), sum(cands)
    stride, ldc16 = Ic + 7, 2 * d + 8
    buf = torch.full((R, stride, ldc16), float('nan'), dtype=torch.bfloat16)           # reserve rows, padding: never read
    buf[:, :Ic, :2 * d] = p['kv'].reshape(R, Ic, 2 * d).to(torch.bfloat16)
    assert torch.equal(buf[:, :Ic, :2 * d].double(), p['kv'].reshape(R, Ic, 2 * d))
    out = torch.full((C * Kq, d), float('nan'), device=dev)
    lse = torch.full((C, H, Kq), float('nan'), device=dev)
    K.attn_fwd_cached_kv16(p['qkv'].float().to(dev), 3 * d, buf.to(dev), ldc16, stride, _req_dev(p, dev), C, H, Ic, n, Kq,
                           hd, out, None, lse)
    torch.cuda.synchronize()
    check(f'kv16 H{H}-{hd}-Ic{Ic}-n{n}-K{Kq} {case}', p['ref'], [p['f32']],
          fwd_outputs(out.double().cpu(), lse.double().cpu()), AE.MARGIN_F32)
