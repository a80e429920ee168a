"""GPU: ot_attn_fwd_cached_lse / ot_attn_bwd_cached against the float64 reference on the expanded problem
(tests/request_attn_ref.py).  Bounds are those tests/test_kernels_gpu.py uses for ot_attn_fwd / ot_attn_bwd."""

import numpy as np
import pytest
import torch

from recommend_amd import kernels as K

import request_attn_ref as RA

pytestmark = pytest.mark.gpu

CANDS = [3, 0, 9, 1, 40]            # an empty request; stacked query counts cross 32 and 64
NK = [(1, 1), (5, 5), (12, 1), (12, 7), (33, 33)]
SENTINEL = 12345.0


def _problem(H, hd, Ic, n, Kq, seed):
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    R, C = len(CANDS), sum(CANDS)
    ld, ldc = 3 * d + 8, 2 * d + 4                      # wider rows than the operands need
    qkv = torch.randn(C * n, ld, generator=g, dtype=torch.float64)
    kv = torch.randn(R * Ic, ldc, generator=g, dtype=torch.float64)
    dout = torch.randn(C * Kq, d, generator=g, dtype=torch.float64)
    req = np.repeat(np.arange(R), CANDS).astype(np.int32)
    return d, R, C, ld, ldc, qkv, kv, dout, req


@pytest.mark.parametrize('Ic', [0, 1, 31, 32, 33, 70])
@pytest.mark.parametrize('H,hd', [(1, 32), (4, 32), (1, 64), (4, 64)])
def test_cached_attention_against_float64(dev, H, hd, Ic):
    check(dev, H, hd, Ic, NK)


@pytest.mark.parametrize('H,hd', [(2, 16), (2, 128)])
def test_cached_attention_other_head_dims(dev, H, hd):
    """The other two supported head dims (their own register and LDS budgets), at one cache length."""
    check(dev, H, hd, 33, [(12, 7), (33, 33)])


def check(dev, H, hd, Ic, shapes):
    for n, Kq in shapes:
        d, R, C, ld, ldc, qkv, kv, dout, req = _problem(H, hd, Ic, n, Kq, seed=1000 * Ic + 10 * n + Kq)
        ref_out, ref_lse, ref_dqkv, ref_dkv = RA.forward_backward(qkv, kv, req, R, H, Ic, n, Kq, dout)
        qkv_d, kv_d, dout_d = qkv.float().to(dev), kv.float().to(dev), dout.float().to(dev)
        # the library indexes an empty cache by pointer arithmetic only: give it a valid base
        kv_p = kv_d if Ic else torch.zeros(1, ldc, device=dev)
        req_d = torch.from_numpy(req).to(dev)
        req_start = torch.searchsorted(req_d, torch.arange(R + 1, device=dev, dtype=torch.int32)).to(torch.int32)
        out = torch.empty(C * Kq, d, device=dev)
        out0 = torch.empty(C * Kq, d, device=dev)
        lse = torch.empty(C, H, Kq, device=dev)
        K.attn_fwd_cached_lse(qkv_d, ld, kv_p, ldc, req_d, C, H, Ic, n, Kq, hd, out, lse)
        K.attn_fwd_cached(qkv_d, ld, kv_p, ldc, req_d, C, H, Ic, n, Kq, hd, out0)
        assert torch.equal(out, out0), (n, Kq)                       # the same forward, bit for bit
        torch.testing.assert_close(out.double().cpu(), ref_out, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(lse.double().cpu(), ref_lse, rtol=1e-5, atol=1e-5)

        runs = []
        for _ in range(2):
            dqkv = torch.full((C * n, ld), SENTINEL, device=dev)
            dkv = torch.full((max(R * Ic, 1), ldc), SENTINEL, device=dev)
            K.attn_bwd_cached(qkv_d, ld, kv_p, ldc, req_start, R, C, H, Ic, n, Kq, hd, out, dout_d, lse, dqkv, dkv)
            runs.append((dqkv, dkv))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (n, Kq)
        dqkv, dkv = runs[0]
        got = dqkv.double().cpu().reshape(C, n, ld)
        want = ref_dqkv.reshape(C, n, 3 * d)
        torch.testing.assert_close(got[:, :, d:3 * d], want[:, :, d:], rtol=1e-4, atol=1e-4)            # dk | dv
        torch.testing.assert_close(got[:, n - Kq:, :d], want[:, n - Kq:, :d], rtol=1e-4, atol=1e-4)     # dq, kept rows
        assert (got[:, :n - Kq, :d] == SENTINEL).all()               # rows without a query: dq not written
        assert (got[:, :, 3 * d:] == SENTINEL).all()                 # the row padding is not touched
        if Ic:
            gkv = dkv.double().cpu()
            torch.testing.assert_close(gkv[:, :2 * d], ref_dkv, rtol=1e-4, atol=1e-4)
            assert (gkv[:, 2 * d:] == SENTINEL).all()
            assert (gkv.reshape(R, Ic, ldc)[1, :, :2 * d] == 0).all()   # the request without candidates: zeros
            # accumulate: the prefilled buffer plus the reference
            pre = torch.randn(R * Ic, ldc, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
            acc = pre.float().to(dev)
            dq2 = torch.full((C * n, ld), SENTINEL, device=dev)
            K.attn_bwd_cached(qkv_d, ld, kv_p, ldc, req_start, R, C, H, Ic, n, Kq, hd, out, dout_d, lse, dq2, acc,
                              accumulate=True)
            assert torch.equal(dq2, dqkv)
            gacc = acc.double().cpu()
            torch.testing.assert_close(gacc[:, :2 * d], pre.float().double()[:, :2 * d] + ref_dkv, rtol=1e-4, atol=1e-4)
            assert torch.equal(gacc[:, 2 * d:], pre.float().double()[:, 2 * d:])
