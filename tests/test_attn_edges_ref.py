"""The saturating / peaked softmax cases of tests/attn_edges_ref.py, proved discriminating on the CPU at every shape
tests/test_attn_softmax_edges_gpu.py runs: the float64 reference is finite, the scores sit where the case says, a
float32 softmax without the max subtraction overflows ('rising') or sums to zero ('all_negative'), the float32
yardstick is non-zero for every output — and a reference that omits the subtraction, or takes the maximum before the
mask, fails the bound the kernels are held to."""

import math

import pytest
import torch

import attn_edges_ref as AE
import kv16_ref as KR
import request_attn_ref as RA

PLAIN = sorted({(shape, sel) for _, _, shape, sel in AE.FWD + AE.BWD})
BF16 = sorted({(shape, sel) for _, mode, shape, sel in AE.FWD + AE.BWD if mode == 'bf16'})


def _sid(p):
    return '-'.join(map(str, p[0])) + ('-sel' if p[1] else '')


def check_scores(case, s, see):
    """s [N, H, Kq, J] float64 scores, see: their visibility."""
    vmax = s[see].max().item()
    if case in ('peaked', 'rising', 'falling'):
        assert 100.0 <= vmax <= 200.0, vmax
    if case == 'all_negative':
        assert vmax <= -110.0, vmax
    sm = s.masked_fill(~see, float('-inf'))
    if case in ('rising', 'falling', 'all_negative'):
        rowmax = torch.softmax(sm, -1).max(-1).values
        assert rowmax.median().item() < 0.9, rowmax.median().item()
    e = torch.exp(sm.float())                                   # float32, no subtraction
    if case == 'rising':
        assert torch.isinf(e).any()
    if case == 'all_negative':
        assert (e.sum(-1) == 0).all()


def check_recompute(p, leaves):
    """The recomputing algorithm is the same operation: in float64 it gives the reference; in float32 it differs."""
    ref = p['ref']
    exact = AE.evaluate_recompute(p['layout'], leaves, p['dout'], torch.float64)
    for a, b in [(exact['out'], ref['out']), (exact['lse'], ref['lse'])] + list(zip(exact['grads'], ref['grads'])):
        assert AE.err(a, b) <= 1e-10 * max(1.0, b.abs().max().item())
    assert all(AE.err(a, b) > 0 for a, b in zip(p['rec32']['grads'], ref['grads']))


def check_problem(p, d):
    ref, f32 = p['ref'], p['f32']
    for t in [ref['out'], ref['lse']] + ref['grads']:
        assert torch.isfinite(t).all()
    check_recompute(p, [p['qkv']])
    assert AE.err(f32['out'], ref['out']) > 0 and AE.err(f32['lse'], ref['lse']) > 0
    for g32, g in zip(f32['grads'], ref['grads']):
        for name, part in AE.split_dqkv(g, d).items():
            if part.shape[1]:
                assert AE.err(AE.split_dqkv(g32, d)[name], part) > 0, name


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('shape,sel', PLAIN, ids=map(_sid, PLAIN))
def test_plain_cases(shape, sel, case):
    B, H, I, Kq, hd = shape
    p = AE.plain_problem(case, B, H, I, Kq, hd, sel)
    assert torch.equal(p['qkv'], p['qkv'].float().double()) and torch.equal(p['dout'], p['dout'].float().double())
    q, k, _, vis = p['layout'](p['qkv'])
    check_scores(case, *AE.scores(q, k, vis))
    check_problem(p, H * hd)


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('shape,sel', BF16, ids=map(_sid, BF16))
def test_bf16_mode_yardstick(shape, sel, case):
    """The bf16 mode's reference (operands rounded to bf16) keeps the cases' properties; the emulation without its
    roundings is the reference (its hand-written backward is right), with them it differs in every output."""
    B, H, I, Kq, hd = shape
    p = AE.plain_problem(case, B, H, I, Kq, hd, sel, operands_bf16=True)
    assert torch.equal(p['qkv'], AE.bf16(p['qkv']))
    q, k, _, vis = p['layout'](p['qkv'])
    s, see = AE.scores(q, k, vis)
    if case == 'peaked':
        assert 100.0 <= s[see].max().item() <= 200.0
    else:
        check_scores(case, s, see)
    ref = p['ref']
    exact = AE.bf16_emulation(p['qkv'], p['dout'], B, H, I, hd, p['qpos'], planes_fwd=False, planes_bwd=False)
    for a, b in [(exact['out'], ref['out']), (exact['lse'], ref['lse']), (exact['grads'][0], ref['grads'][0])]:
        assert AE.err(a, b) <= 1e-11 * max(1.0, b.abs().max().item())
    for fwd, bwd in [(True, True), (True, False)]:
        emu = AE.bf16_emulation(p['qkv'], p['dout'], B, H, I, hd, p['qpos'], planes_fwd=fwd, planes_bwd=bwd)
        assert torch.isfinite(emu['out']).all() and torch.isfinite(emu['lse']).all()
        assert torch.isfinite(emu['grads'][0]).all()
        assert AE.err(emu['out'], ref['out']) > 0 and AE.err(emu['lse'], ref['lse']) > 0
        for name, part in AE.split_dqkv(emu['grads'][0], H * hd).items():
            assert AE.err(part, AE.split_dqkv(ref['grads'][0], H * hd)[name]) > 0, name


@pytest.mark.parametrize('case', AE.MASKED_CASES)
@pytest.mark.parametrize('shape', AE.MASKED, ids=lambda s: '-'.join(map(str, s)))
def test_masked_cases(shape, case):
    B, H, I, Kq, hd = shape
    p = AE.plain_problem(case, B, H, I, Kq, hd, masked=True)
    valid = p['valid']
    assert 0.55 < valid.float().mean().item() < 0.85
    q, k, _, vis = p['layout'](p['qkv'])
    s, see = AE.scores(q, k, vis)
    check_problem(p, H * hd)
    if case == 'rising':
        check_scores(case, s, see)
        return
    # dominant_invalid: a query at a valid position sees nothing above 10; the keys the mask hides from it (causally
    # visible, invalid) reach past 100
    causal = AE.visibility(p['qpos'], I)[:, None].expand_as(s)
    at_valid = valid[torch.arange(B)[:, None], p['qpos']][:, None, :, None].expand_as(s)
    assert s[see & at_valid].max().item() < 10.0
    hidden = causal & ~see & at_valid
    assert hidden.any() and s[hidden].max().item() > 100.0
    rows = hidden.any(-1)                                       # every such query that has a hidden key at all
    assert (s.masked_fill(~hidden, float('-inf')).max(-1).values[rows] > 100.0).all()


def _cached_scores(p):
    q, k, _, vis = p['layout'](p['qkv'], p['kv'])
    return AE.scores(q, k, vis)


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('H,hd,Ic,n,Kq', AE.CACHED)
def test_cached_cases(H, hd, Ic, n, Kq, case):
    p = AE.cached_problem(case, AE.CANDS, H, Ic, n, Kq, hd)
    s, see = _cached_scores(p)
    check_scores(case, s, see)
    d = H * hd
    ref = p['ref']
    for t in [ref['out'], ref['lse']] + ref['grads']:
        assert torch.isfinite(t).all()
    for name in ('out', 'lse'):
        assert AE.err(p['f32'][name], ref[name]) > 0
    assert all(AE.err(a, b) > 0 for a, b in zip(p['f32']['grads'], ref['grads']))
    check_recompute(p, [p['qkv'], p['kv']])
    # where the dominant key lies: the cache for 'falling', the own rows for 'rising'
    top = s.masked_fill(~see, float('-inf')).argmax(-1)
    if case == 'falling':
        assert (top < Ic).all()
    if case == 'rising':                                        # (the first of Kq == n queries sees one own row only)
        assert (top[..., -1] >= Ic).all()
    # the same operation as tests/request_attn_ref.py states it
    C = sum(AE.CANDS)
    out, lse, dqkv, dkv = RA.forward_backward(p['qkv'], p['kv'], p['req'], len(AE.CANDS), H, Ic, n, Kq, p['dout'])
    for a, b in [(out, ref['out']), (lse, ref['lse']), (dqkv, ref['grads'][0]), (dkv, ref['grads'][1])]:
        assert AE.err(a, b) <= 1e-11 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize('case', AE.CASES + ('dominant_invalid',))
def test_cached_masked_cases(case):
    cands, H, hd, Ic, n, Kq = AE.CACHED_MASKED
    p = AE.cached_problem(case, cands, H, Ic, n, Kq, hd, masked=True)
    s, see = _cached_scores(p)
    assert torch.isfinite(p['ref']['out']).all() and torch.isfinite(p['ref']['lse']).all()
    assert AE.err(p['f32']['out'], p['ref']['out']) > 0 and AE.err(p['f32']['lse'], p['ref']['lse']) > 0
    if case != 'dominant_invalid':
        check_scores(case, s, see)
        return
    assert s[see].max().item() < 10.0                           # own rows are valid: every query sits at a valid position
    hidden = ~see & AE.visibility(AE.tail_qpos(s.shape[0], Ic + n, Kq), Ic + n)[:, None].expand_as(s)
    assert (s.masked_fill(~hidden, float('-inf')).max(-1).values > 100.0).all()


@pytest.mark.parametrize('case', AE.CASES)
@pytest.mark.parametrize('cands,H,hd,Ic,n,Kq', AE.KV16)
def test_kv16_cases(cands, H, hd, Ic, n, Kq, case):
    p = AE.cached_problem(case, cands, H, Ic, n, Kq, hd, cache_bf16=True)
    assert torch.equal(p['kv'], AE.bf16(p['kv']))
    check_scores(case, *_cached_scores(p))
    assert AE.err(p['f32']['out'], p['ref']['out']) > 0 and AE.err(p['f32']['lse'], p['ref']['lse']) > 0
    # the same operation as tests/kv16_ref.py states it
    out, lse = KR.cached_attention_ref(p['qkv'].float(), p['kv'].to(torch.bfloat16), Ic, p['req'], H, Ic, n, Kq, H * hd)
    assert AE.err(out.reshape(-1, H * hd), p['ref']['out']) <= 1e-11 and AE.err(lse, p['ref']['lse']) <= 1e-11


# ------------------------------------------------------------------------------------------------ self-checks
def no_subtraction(q, k, v, vis):
    """float32 softmax without the running-max subtraction."""
    q, k, v = q.float(), k.float(), v.float()
    s = (torch.einsum('nqhe,nkhe->nhqk', q, k) / math.sqrt(q.shape[-1])).masked_fill(~vis[:, None], float('-inf'))
    e = torch.exp(s)
    l = e.sum(-1, keepdim=True)
    return torch.einsum('nhqk,nkhe->nqhe', e / l, v).reshape(q.shape[0], q.shape[1], -1), torch.log(l)[..., 0]


def max_before_mask(q, k, v, vis):
    """float32 softmax whose maximum is taken over every key, the masked ones included."""
    q, k, v = q.float(), k.float(), v.float()
    s = torch.einsum('nqhe,nkhe->nhqk', q, k) / math.sqrt(q.shape[-1])
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m).masked_fill(~vis[:, None], 0.0)
    l = e.sum(-1, keepdim=True)
    return torch.einsum('nhqk,nkhe->nqhe', e / l, v).reshape(q.shape[0], q.shape[1], -1), (m + torch.log(l))[..., 0]


def passes(fn, p):
    """Would ``fn`` in a kernel's place pass the GPU file's check of out and lse at the f32 margin?"""
    out, lse = fn(*p['layout'](p['qkv']))
    ref, f32 = p['ref'], p['f32']
    out = out.reshape(ref['out'].shape).double()
    return (AE.within(out, ref['out'], AE.err(f32['out'], ref['out']), AE.MARGIN_F32)
            and AE.within(lse.double(), ref['lse'], AE.err(f32['lse'], ref['lse']), AE.MARGIN_F32))


def test_missing_subtraction_is_caught():
    """What randn inputs cannot see: the softmax without the subtraction passes on them, and fails 'rising' and
    'all_negative'."""
    B, H, I, Kq, hd = 2, 4, 140, 140, 32
    assert passes(no_subtraction, AE.plain_problem('randn', B, H, I, Kq, hd))
    assert not passes(no_subtraction, AE.plain_problem('rising', B, H, I, Kq, hd))
    assert not passes(no_subtraction, AE.plain_problem('all_negative', B, H, I, Kq, hd))


def test_maximum_before_mask_is_caught():
    """The maximum taken before the mask passes on randn, and fails 'rising' at Kq == I (the causally masked keys hold
    the largest scores) and 'dominant_invalid' (the padding keys do)."""
    B, H, I, Kq, hd = 2, 4, 300, 300, 32
    assert passes(max_before_mask, AE.plain_problem('randn', B, H, I, Kq, hd))
    assert not passes(max_before_mask, AE.plain_problem('rising', B, H, I, Kq, hd))
    B, H, I, Kq, hd = 3, 2, 70, 70, 32
    assert passes(max_before_mask, AE.plain_problem('randn', B, H, I, Kq, hd, masked=True))
    assert not passes(max_before_mask, AE.plain_problem('dominant_invalid', B, H, I, Kq, hd, masked=True))
