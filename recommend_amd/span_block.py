"""What the two-stage paths share (paper §3.5.1): cached serving (recommend_amd/serving.py) and request-grouped
training (recommend_amd/request_train.py) both run every layer as an S span (once per request) and an N span (once
per candidate, its queries over the request's S-side K/V).  Here: the per-layer split of the pyramid schedule, the
plain-form block forward on one span, the S rows of a tokenizer output, and the check of ``req``."""

from __future__ import annotations

from typing import Dict, List

import torch

from . import kernels as K
from ._lib import OT_AX_GELU, OT_AX_RMSNORM, OT_EPI_BIAS, OT_EPI_DROPOUT, OT_EPI_RESIDUAL, OT_GEMM_NT
from .block import RMS_EPS


def request_schedule(cfg, L_S: int) -> List[Dict]:
    """The two-stage split of every layer (serving and request-grouped training): S rows s, N rows n, kept S
    rows kS, kept N rows kN (kS + kN = the layer's keep; the tail keep takes the N rows first)."""
    L_NS = cfg.num_ns_tokens
    sched = cfg.pyramid_schedule(L_S + L_NS)
    out, s, n = [], L_S, L_NS
    for l, e in enumerate(sched):
        keep = e['keep'] if l < len(sched) - 1 else 1        # only the last token is read (model.py:390)
        kN = min(keep, n)
        kS = keep - kN
        out.append({'I': s + n, 's': s, 'n': n, 'kS': kS, 'kN': kN})
        s, n = kS, kN
    return out


def s_rows(x0: torch.Tensor, plan) -> torch.Tensor:
    """The S tokens [B*L_S, d] of a tokenizer output x0 [B*L0, d] ([S ; NS] per sample)."""
    B, L0, L_S = plan['B'], plan['L0'], plan['L_S']
    d = x0.shape[1]
    return x0.view(B, L0, d)[:, :L_S].reshape(B * L_S, d)


def s_rows_grad(dxs: torch.Tensor, plan) -> torch.Tensor:
    """``s_rows`` backwards: dx0 [B*L0, d] holding dxs in the S rows and zeros in the NS rows."""
    B, L0, L_S = plan['B'], plan['L0'], plan['L_S']
    d = dxs.shape[1]
    dx0 = torch.zeros(B, L0, d, device=dxs.device)
    dx0[:, :L_S] = dxs.reshape(B, L_S, d)
    return dx0.view(B * L0, d)


def check_req(who: str, req, R: int, C: int, ordered: bool) -> None:
    """``req`` [C]: integer request indices in [0, R), non-decreasing when ``ordered``.  Checked before any launch
    (the kernels index the K/V rows with req unchecked): host indices directly, device indices with one small
    read-back."""
    t = torch.as_tensor(req)
    if t.dim() != 1 or t.numel() != C:
        raise ValueError(f'{who}: req has shape {tuple(t.shape)}, expected ({C},) — one request index per candidate')
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f'{who}: req is {t.dtype}; integer request indices are expected')
    if C == 0:
        return
    t = t.to(torch.int64)
    stats = [t.min(), t.max()] + ([(t[1:] < t[:-1]).sum()] if ordered else [])
    lo, hi, *descents = (int(v) for v in torch.stack(stats).cpu())
    if lo < 0 or hi >= R:
        raise ValueError(f'{who}: request index out of range [0, {R}) (min {lo}, max {hi})')
    if ordered and descents[0]:
        raise ValueError(f'{who}: req must be non-decreasing (candidates grouped by request); '
                         f'{descents[0]} descent(s)')


def span_forward(m, l: int, x: torch.Tensor, B: int, I: int, Kq: int, p0: int, I_full: int, *, cached: bool,
                 kv=None, req=None, R: int = 0, seed: int = 0, rate: float = 0.0, for_backward: bool = False,
                 valid=None, kv16=None, Ic: int = 0):
    """OneTransBlock.call (model.py:186-200) on B spans of I rows (positions p0.. of a layer of I_full tokens),
    keeping the last Kq; plain kernel forms.  Returns (x2 [B*Kq, d], qkv [B*I, 3d], saved); Kq = 0: only the K/V
    rows of qkv are produced and x2 is None.

    ``cached`` False: self-attention (the S span).  True: the span's queries attend over ``kv``'s K/V columns
    ([R*Ic, 3d], the rows of request ``req[b]``; None with nothing cached) and their own rows (the N span).
    ``rate`` > 0: dropout on the two branch outputs under ``seed``, sites 2l and 2l+1.
    ``for_backward``: the forward of a training step: the Q columns of rows without a query are zeroed (the
    backward's weight gradient reads every column), the cached attention writes its lse, and ``saved`` is what the
    backward reads (x, rstd1[, qkv, o, lse, x1, rstd2, u]).
    ``valid`` (seq_padding_mask): the key-padding mask as (uint8 tensor, element offset, row stride) — of the span's
    own I keys when not ``cached``, of the Ic cached rows ([R, .]) when ``cached`` (the span's own rows are valid).
    ``kv16`` (serving with a bf16 request cache), instead of ``kv`` when ``cached``: (bfloat16 tensor [R, cap, ld16],
    cap) — request r's ``Ic`` cached rows are the first Ic of its cap rows, K at col 0 and V at col d; ``Ic`` is given
    (the buffer may hold reserve rows).  Inference only: it raises with ``for_backward``."""
    if kv16 is not None and (for_backward or not cached or kv is not None):
        raise ValueError('span_forward: kv16 (a bf16 request cache) is an alternative to kv for cached inference; '
                         'the backward reads f32 K/V rows')
    cfg = m.config
    d, f, H = cfg.hidden_dim, cfg.ffn_dim, cfg.num_heads
    hd = d // H
    dev = x.device
    mp = m.maps(B, I, max(Kq, 1), p0, I_full)
    ma, mt = mp['all'].to(dev), mp['tail'].to(dev)
    na, nt = mp['all'].ntiles, mp['tail'].ntiles
    dflag = OT_EPI_DROPOUT if rate > 0 else 0
    tail = (Kq, I)
    wqkv, wo = m.pT(f'blk.{l}.wqkv'), m.pT(f'blk.{l}.wo')
    w1, b1, w2, b2 = m.pT(f'blk.{l}.w1'), m.p(f'blk.{l}.b1'), m.pT(f'blk.{l}.w2'), m.p(f'blk.{l}.b2')
    g1, g2 = m.p(f'blk.{l}.norm1'), m.p(f'blk.{l}.norm2')
    rstd1 = torch.empty(B * I, device=dev)
    K.rmsnorm_fwd(x, d, B * I, d, rstd1, eps=RMS_EPS)
    qkv = torch.empty(B * I, 3 * d, device=dev)
    if for_backward and Kq < I:
        qkv[:, :d].zero_()                       # rows without a query
    # K/V for every row (weight cols d..3d of each group's [d, 3d] bank), Q for the kept rows
    K.gemm(OT_GEMM_NT, x, d, d, ma['rows'][0], (wqkv, d * d), 3 * d * d, d, 2 * d, ma['tile_group'], na,
           (qkv, d), 3 * d, ma['rows'][0], a_xform=OT_AX_RMSNORM, rstd=rstd1, gamma=g1, m_rows=mp['all'].nrows)
    if Kq == 0:
        return None, qkv, (x, rstd1)
    K.gemm(OT_GEMM_NT, x, d, d, mt['rows'][0], wqkv, 3 * d * d, d, d, mt['tile_group'], nt, qkv, 3 * d,
           mt['rows'][0], a_xform=OT_AX_RMSNORM, rstd=rstd1, gamma=g1, m_rows=mp['tail'].nrows)
    o = torch.empty(B * Kq, d, device=dev)
    lse = torch.empty(B * H * Kq, device=dev) if for_backward or not cached else None
    if cached and kv16 is not None:
        buf, req_stride = kv16
        K.attn_fwd_cached_kv16(qkv, 3 * d, buf, buf.shape[-1], req_stride, req, B, H, Ic, I, Kq, hd, o,
                               valid if Ic > 0 else None, lse)
    elif cached:
        Ic = kv.shape[0] // R if kv is not None else 0
        if valid is not None:
            K.attn_fwd_cached_masked(qkv, 3 * d, (kv, d) if kv is not None else None, 3 * d, req, B, H, Ic, I, Kq, hd,
                                     o, valid if Ic > 0 else None, lse)
        else:
            K.attn_fwd_cached(qkv, 3 * d, (kv, d) if kv is not None else None, 3 * d, req, B, H, Ic, I, Kq, hd, o, lse)
    elif valid is not None:
        K.attn_fwd_masked(qkv, 3 * d, B, H, I, Kq, hd, o, lse, valid)
    else:
        K.attn_fwd(qkv, 3 * d, B, H, I, Kq, hd, o, lse)
    # x1 = x[tail] + drop(o @ Wo)
    x1 = torch.empty(B * Kq, d, device=dev)
    K.gemm(OT_GEMM_NT, o, d, d, mt['rows'][1], wo, 0, d, d, mt['tile_group'], nt, x1, d, mt['rows'][1],
           epi=OT_EPI_RESIDUAL | dflag, res=x, ldres=d, res_tok=1, seed=seed, site=2 * l, drop=rate, tail=tail,
           m_rows=mp['tail'].nrows)
    rstd2 = torch.empty(B * Kq, device=dev)
    K.rmsnorm_fwd(x1, d, B * Kq, d, rstd2, eps=RMS_EPS)
    # u = norm2(x1) @ W1[g] + b1[g]; x2 = x1 + drop(gelu(u) @ W2[g] + b2[g])
    u = torch.empty(B * Kq, f, device=dev)
    K.gemm(OT_GEMM_NT, x1, d, d, mt['rows'][1], w1, d * f, d, f, mt['tile_group'], nt, u, f, mt['rows'][1],
           a_xform=OT_AX_RMSNORM, rstd=rstd2, gamma=g2, bias=b1, bias_gstride=f, epi=OT_EPI_BIAS,
           m_rows=mp['tail'].nrows)
    x2 = torch.empty(B * Kq, d, device=dev)
    K.gemm(OT_GEMM_NT, u, f, f, mt['rows'][1], w2, f * d, f, d, mt['tile_group'], nt, x2, d, mt['rows'][1],
           a_xform=OT_AX_GELU, bias=b2, bias_gstride=d, epi=OT_EPI_BIAS | OT_EPI_RESIDUAL | dflag, res=x1,
           ldres=d, res_tok=0, seed=seed, site=2 * l + 1, drop=rate, tail=tail, m_rows=mp['tail'].nrows)
    return x2, qkv, (x, rstd1, qkv, o, lse, x1, rstd2, u)
