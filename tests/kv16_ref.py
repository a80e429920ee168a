"""Yardsticks for the bf16 request cache of serving (no GPU): the rounding a stored row gets and the float64
cached attention over [bf16 cached rows ; f32 own rows]."""

import math

import torch


def round_bf16(x):
    """f32 -> bf16 as a cache row is stored: round to nearest even, NaN stays NaN, past the range +-inf."""
    return x.to(torch.bfloat16)


def bits16(x):
    """bf16 tensor -> its bit patterns (int32, 0 .. 0xFFFF)."""
    return x.view(torch.int16).to(torch.int32) & 0xFFFF


def f32_from_bits(words):
    """f32 values from their bit patterns (Python ints, 0 .. 2^32 - 1)."""
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(torch.float32)


# (f32 bits, bf16 bits): ties to even down and up, the largest finite f32, -0, subnormals, +-inf
SPECIALS = [(0x3F808000, 0x3F80),      # 1 + 2^-8: halfway, the even neighbour is below
            (0x3F818000, 0x3F82),      # 1 + 3 * 2^-8: halfway, the even neighbour is above
            (0x3F808001, 0x3F81),      # just past halfway
            (0x7F7FFFFF, 0x7F80),      # past the bf16 range: +inf
            (0xFF7FFFFF, 0xFF80),
            (0x80000000, 0x8000),      # -0 keeps its sign
            (0x00010000, 0x0001),      # a subnormal that bf16 holds
            (0x00008000, 0x0000),      # a subnormal halfway to the smallest one: ties to even, 0
            (0x00018000, 0x0002),
            (0x7F800000, 0x7F80), (0xFF800000, 0xFF80)]


def cached_attention_ref(qkv, kv16, req_stride, req, H, Ic, n, Kq, d, cache_valid=None):
    """qkv [C*n, >= 3d] f32 (q | k | v, the candidates' own rows); kv16 [R*req_stride, >= 2d] bfloat16 (k | v; request
    r's cached key j < Ic is row r*req_stride + j, anything else in the tensor is never read); req [C];
    cache_valid None or bool [R, >= Ic] over the cached rows (own rows are valid).  Query j of candidate c sits at
    position Ic + n - Kq + j of [cached ; own].  float64 out [C, Kq, d], lse [C, H, Kq]."""
    assert kv16.dtype == torch.bfloat16
    C, hd = qkv.shape[0] // n, d // H
    R = kv16.shape[0] // req_stride
    req = torch.as_tensor(req, dtype=torch.long)
    own = qkv[:, :3 * d].double().reshape(C, n, 3 * d)
    c = kv16.reshape(R, req_stride, -1)[:, :Ic, :2 * d].double()         # widening bf16 is exact
    keys = torch.cat([c[req][..., :d], own[..., d:2 * d]], 1).reshape(C, Ic + n, H, hd)
    vals = torch.cat([c[req][..., d:], own[..., 2 * d:]], 1).reshape(C, Ic + n, H, hd)
    qs = own[:, n - Kq:, :d].reshape(C, Kq, H, hd)
    s = torch.einsum('cqhe,ckhe->chqk', qs, keys) / math.sqrt(hd)
    qpos = Ic + n - Kq + torch.arange(Kq)
    see = (torch.arange(Ic + n)[None, :] <= qpos[:, None])[None].expand(C, Kq, Ic + n).clone()
    if cache_valid is not None and Ic > 0:
        see[:, :, :Ic] &= torch.as_tensor(cache_valid, dtype=torch.bool)[req][:, None, :Ic]
    s = s.masked_fill(~see[:, None], float('-inf'))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = torch.einsum('chqk,ckhe->cqhe', p, vals).reshape(C, Kq, d)
    return out, lse
