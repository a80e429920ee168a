"""CPU: the yardsticks of the bf16 request cache (tests/kv16_ref.py) checked against hand-written cases, the cache's
byte formula, and the new entry points' names and arity."""

import os

import numpy as np
import pytest
import torch

import kv16_ref as KR
import request_attn_ref as RA
from recommend_amd import _lib
from recommend_amd import kernels as K
from recommend_amd.serving import CACHE_DTYPES, OneTransServer, RequestCache, bf16_cache_nbytes
from recommend_amd.span_block import request_schedule
from test_abi_layout import _prototypes
from test_model_gpu import small_criteo


def test_round_bf16_bit_patterns():
    x = KR.f32_from_bits([w for w, _ in KR.SPECIALS])
    got = KR.bits16(KR.round_bf16(x)).tolist()
    assert got == [b for _, b in KR.SPECIALS], [hex(g) for g in got]
    assert torch.isnan(KR.round_bf16(torch.tensor([float('nan')])).float()).all()
    # a NaN whose payload sits only in the low 16 bits must not round to inf
    assert torch.isnan(KR.round_bf16(KR.f32_from_bits([0x7F800001, 0xFF80FFFF])).float()).all()
    assert torch.equal(KR.round_bf16(torch.tensor([-0.0])).float().signbit(), torch.tensor([True]))


def test_cached_attention_ref_matches_request_ref_on_representable_cache():
    """Every cached value exactly a bf16, every row valid: the plain float64 cached attention, with the request
    stride, padding rows and padding columns of the bf16 layout in place (NaN: they must not be read)."""
    R, C, H, hd, n, Kq, Ic, stride = 3, 5, 2, 16, 4, 3, 9, 14
    d = H * hd
    torch.manual_seed(0)
    req = [0, 2, 1, 2, 0]
    kv = torch.randn(R, Ic, 2 * d).bfloat16()
    buf = torch.full((R, stride, 2 * d + 8), float('nan'), dtype=torch.bfloat16)
    buf[:, :Ic, :2 * d] = kv
    own = torch.randn(C * n, 3 * d + 4)
    out, lse = KR.cached_attention_ref(own, buf.reshape(R * stride, -1), stride, req, H, Ic, n, Kq, d)
    o3 = own[:, :3 * d].double().reshape(C, n, 3 * d)
    ref, ref_lse = RA.forward(o3[..., :d], o3[..., d:2 * d], o3[..., 2 * d:], kv[..., :d].double(), kv[..., d:].double(),
                              req, H, Kq)
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse, ref_lse, rtol=1e-12, atol=1e-12)
    # all-ones validity is the same thing; a masked row changes the result and equals dropping that row's weight
    out1, _ = KR.cached_attention_ref(own, buf.reshape(R * stride, -1), stride, req, H, Ic, n, Kq, d,
                                      np.ones((R, Ic), bool))
    torch.testing.assert_close(out1, out, rtol=0, atol=0)
    cv = np.ones((R, Ic), bool)
    cv[1] = False                                            # request 1: nothing cached is visible
    out2, lse2 = KR.cached_attention_ref(own, buf.reshape(R * stride, -1), stride, req, H, Ic, n, Kq, d, cv)
    alone, alone_lse = RA.forward(o3[2:3, :, :d], o3[2:3, :, d:2 * d], o3[2:3, :, 2 * d:], kv[:1, :0, :d].double(),
                                  kv[:1, :0, d:].double(), [0], H, Kq)      # candidate 2 over its own rows only
    torch.testing.assert_close(out2[2:3], alone, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse2[2:3], alone_lse, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(out2[0], out[0], rtol=0, atol=0)
    assert torch.isfinite(out2).all() and torch.isfinite(lse2).all()


def test_byte_formula():
    """R · Σ_l cap_l · 2d · 2, cap_l = Ic_l + reserve, against the two-stage schedule."""
    flat = small_criteo('tail', layers=3, d=64, H=4)
    L_S = flat.seq_token_count(flat._seq_lens)
    for R, reserve in [(1, 0), (3, 0), (3, 8)]:
        assert bf16_cache_nbytes(flat, R, L_S, reserve) == R * 3 * (L_S + reserve) * 2 * 64 * 2   # no pruning: Ic = L_S
    pyr = small_criteo('tail', pyramid=True, layers=3, d=128, H=4, f=256, Lns=12, seq_lens=(20, 20, 20))
    L_S = pyr.seq_token_count(pyr._seq_lens)
    sched = request_schedule(pyr, L_S)
    s = [e['s'] for e in sched]
    assert s[0] == L_S and s[-1] < s[0] and all(a >= b for a, b in zip(s, s[1:]))     # the pyramid shrinks the S side
    for R, reserve in [(2, 0), (2, 5)]:
        want = sum(R * (e['s'] + reserve) * 2 * 128 * 2 for e in sched)
        assert bf16_cache_nbytes(pyr, R, L_S, reserve) == want
    # against the fp32 cache (whole qkv rows, 3d floats): a third
    assert 3 * bf16_cache_nbytes(pyr, 2, L_S) == sum(2 * e['s'] * 3 * 128 * 4 for e in sched)


def test_cache_object_nbytes_and_dtype():
    d = 8
    f32 = RequestCache(2, 5, [{'Ic': 5, 'kv': torch.zeros(10, 3 * d)}, {'Ic': 0, 'kv': None}])
    assert f32.dtype == 'fp32' and f32.nbytes() == 10 * 3 * d * 4
    buf = torch.zeros(2, 7, 2 * d, dtype=torch.bfloat16)
    b16 = RequestCache(2, 5, [{'Ic': 5, 'kv16': buf, 'cap': 7, 'high': [5]}], dtype='bf16')
    assert b16.dtype == 'bf16' and b16.nbytes() == 2 * 7 * 2 * d * 2
    assert CACHE_DTYPES == ('fp32', 'bf16')


def test_new_names_and_arity():
    protos = _prototypes()
    for name in ('ot_kv_pack_bf16', 'ot_attn_fwd_cached_kv16'):
        assert name in _lib.SIGNATURES and name in protos
        assert len(protos[name]) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.header_symbols()
    assert len(protos['ot_kv_pack_bf16']) == 10 and len(protos['ot_attn_fwd_cached_kv16']) == 17
    assert callable(K.kv_pack_bf16) and callable(K.attn_fwd_cached_kv16)
    import inspect
    from recommend_amd.serving import OneTransInferenceEngine
    from recommend_amd.span_block import span_forward
    assert inspect.signature(span_forward).parameters['kv16'].default is None
    assert inspect.signature(OneTransServer.__init__).parameters['cache_dtype'].default == 'fp32'
    assert inspect.signature(OneTransInferenceEngine.__init__).parameters['cache_dtype'].default == 'fp32'
    assert inspect.signature(OneTransServer.encode_requests).parameters['reserve'].default == 0


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')
def test_abi_refusals_without_a_device():
    """Argument checks come before any launch, so they need no GPU."""
    d = 64
    ok = dict(ld=3 * d, R=1, rows=4, d=d, ldc16=2 * d, stride=4, row0=0)

    def pack(**kw):
        a = {**ok, **kw}
        _lib.call('ot_kv_pack_bf16', 16, a['ld'], a['R'], a['rows'], a['d'], 16, a['ldc16'], a['stride'], a['row0'], None)

    for bad in (dict(ldc16=2 * d + 4), dict(ldc16=2 * d - 8), dict(stride=3), dict(row0=1), dict(ld=3 * d + 2),
                dict(ld=3 * d - 4)):
        with pytest.raises(_lib.OneTransHipError):
            pack(**bad)
    with pytest.raises(_lib.OneTransHipError, match='null'):
        _lib.call('ot_kv_pack_bf16', None, 3 * d, 1, 4, d, 16, 2 * d, 4, 0, None)
    pack(R=0)                                                # nothing to do: OT_OK, no launch

    def attn(ldc16=2 * d, stride=8, Ic=8, hd=32, ld=3 * d, kv=16, C=0):
        _lib.call('ot_attn_fwd_cached_kv16', 16, ld, kv, ldc16, stride, 16, C, d // hd if d % hd == 0 else 2, Ic, 4, 4,
                  hd, None, 0, 16, None, None)

    for bad in (dict(ldc16=2 * d + 4), dict(ldc16=2 * d - 8), dict(stride=7), dict(hd=48), dict(ld=3 * d + 2),
                dict(ld=3 * d - 4), dict(kv=None)):
        with pytest.raises(_lib.OneTransHipError):
            attn(**bad)
    attn()                                                   # C == 0: OT_OK, no launch
    attn(Ic=0, kv=None, stride=0, ldc16=0)                   # nothing cached: no cache operand needed
