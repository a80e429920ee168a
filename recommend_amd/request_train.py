"""Request-grouped training (paper §3.5.1, the two-stage request-level scheme applied to training).

The C candidates of a batch belong to R requests; the samples of one request share their S tokens (the
behaviour sequences) and differ only in their NS tokens.  Every layer is therefore run as two spans:

* the S span: R spans of s rows at positions 0.. of the layer, self-attending causally (``ot_attn_fwd`` /
  ``ot_attn_bwd``) — once per request instead of once per candidate;
* the N span: C spans of n rows at positions s.., whose queries attend over their request's S-span K/V
  and their own rows (``ot_attn_fwd_cached_lse`` / ``ot_attn_bwd_cached``).  The backward's gradient of the
  S-span K/V is the sum over the request's candidates; the S span adds it to its own dK/dV.

The result equals ``OneTransModel.forward_probs`` / ``train_step`` on the expanded batch
(``data.expand_requests``: each candidate paired with a copy of its request's sequences) up to fp32
summation order.  The spans use the plain kernel forms (no weight images, fused norms, pair bounds or
bf16 side outputs); the default path is untouched.

Dropout draws its own masks here: a span's element (b, p, col) hashes its span-local index
(b*I + p)*d + col (b the request of an S span, the candidate of an N span; I = s or n), sites 2l and 2l+1
as in the default path; the S span uses the layer seed, the N span the layer seed + ``N_SEED_OFFSET``.
"""

from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch

from . import kernels as K
from ._lib import OT_AX_GELU, OT_AX_RMSNORM, OT_EPI_GELU_BWD, OT_GEMM_NT
from .block import _wgrad_single, layer_seed
from .model import _Head, _Tokenize
from .span_block import check_req, request_schedule, s_rows, s_rows_grad, span_forward

N_SEED_OFFSET = 0x632BE5AB        # odd: the N span's dropout seed is the layer seed plus this (mod 2^32)


def n_span_seed(seed: int) -> int:
    return (seed + N_SEED_OFFSET) & 0xFFFFFFFF


def check_supported(m) -> None:
    """Request-grouped training runs the tail keep in the f32 / split arithmetic on one device."""
    cfg = m.config
    if getattr(cfg, 'pyramid_select', 'tail') != 'tail':
        raise ValueError("forward_requests: pyramid_select must be 'tail' (a score-based keep would depend on the "
                         "NS tokens' positions in every layer)")
    if m.attn_fp8 or m.matmul == 'bf16':
        raise NotImplementedError("forward_requests: compute_dtype 'bf16' / 'fp8attn' is not supported (the cached "
                                  'attention backward is native f32)')
    if m.recompute:
        raise NotImplementedError('forward_requests: recompute_blocks is not supported')
    if getattr(m, 'padding_mask', False):
        raise NotImplementedError('forward_requests: seq_padding_mask is not supported (the cached attention backward, '
                                  'ot_attn_bwd_cached, carries no padding mask)')
    if m.sharded:
        raise NotImplementedError('forward_requests: a row-sharded table is not supported')
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError('forward_requests: data-parallel runs (world size > 1) are not supported')


# =============================================================================== tokenizer
class _TokenizeRequests(torch.autograd.Function):
    """R requests' S tokens (the S-only plan) and C candidates' NS tokens (the NS-only plan) as one autograd
    node: (xS [R*L_S, d], xN [C*L_NS, d]).  One backward serves both plans, so the tokenizer gradients and
    the pending embedding-row gradients of both ('emb.seq_item' from the S plan, 'emb.ns' from the N plan)
    survive each other."""

    @staticmethod
    def forward(ctx, flat, m, plan_s, plan_n):
        cs, cn = SimpleNamespace(), SimpleNamespace()
        x0s = _Tokenize.forward(cs, flat, m, plan_s)            # [R*L0, d]; the NS rows are zero
        xn = _Tokenize.forward(cn, flat, m, plan_n)             # [C*L_NS, d]
        ctx.m, ctx.cs, ctx.cn = m, cs, cn
        return s_rows(x0s, plan_s), xn

    @staticmethod
    def backward(ctx, dxs, dxn):
        m, cs, cn = ctx.m, ctx.cs, ctx.cn
        with K.precision(m.matmul):
            # the S plan first: it writes tok.seq.* / tok.sep and (no NS fields) clears tok.ns.* unless the
            # model accumulates; the N plan then adds its tok.ns.* and leaves the absent sequence parts alone
            _Tokenize._backward(cs, s_rows_grad(dxs, cs.plan))
            pending = m._pending_sparse
            acc = m.accumulate_grads
            m.accumulate_grads = True
            try:
                _Tokenize._backward(cn, dxn)
            finally:
                m.accumulate_grads = acc
            m._pending_sparse = pending + m._pending_sparse
        return None, None, None, None


# =============================================================================== one span of a block
class _SpanBlock(torch.autograd.Function):
    """OneTransBlock.call (model.py:186-200) on B spans of I rows at positions p0.. of a layer of I_full tokens,
    keeping the last Kq rows; plain kernel forms.

    S span (``kv`` None): self-attention; returns (x2 [B*Kq, d], qkv [B*I, 3d]) — qkv is differentiable, its
    incoming gradient (the N span's dK/dV) is added to the span's own before the Wqkv weight gradient and the QKV
    dgrad.  Kq = 0: only the K/V projection runs (x2 is empty).
    N span (``kv`` = the S span's qkv, or None with Ic = 0): cached attention against kv's K/V columns;
    returns x2.

    ``state['written']``: the layers whose weight gradients this backward pass has written — the first span
    of a layer to run its backward writes (honouring ``m.accumulate_grads``), the second accumulates."""

    @staticmethod
    def forward(ctx, flat, x, kv, m, l, span, B, I, Kq, p0, I_full, seed, training, req, req_start, R, state):
        cached = span == 'N'
        rate = m.config.dropout_rate if training else 0.0
        x2, qkv, saved = span_forward(m, l, x, B, I, Kq, p0, I_full, cached=cached, kv=kv, req=req, R=R, seed=seed,
                                      rate=rate, for_backward=True)
        ctx.m, ctx.l, ctx.span, ctx.dims = m, l, span, (B, I, Kq, p0, I_full, R)
        ctx.seed, ctx.rate, ctx.state = seed, rate, state
        ctx.has_kv = kv is not None
        if Kq == 0:
            ctx.save_for_backward(*saved)
            x2 = x.new_empty(0)
            ctx.mark_non_differentiable(x2)
            return x2, qkv
        if cached:
            ctx.save_for_backward(*saved, req_start, *([kv] if kv is not None else []))
            return x2
        ctx.save_for_backward(*saved)
        return x2, qkv

    @staticmethod
    def backward(ctx, *grads):
        # the autograd engine runs this on its own thread: enter the model's precision there
        with K.precision(ctx.m.matmul):
            return _SpanBlock._backward(ctx, *grads)

    @staticmethod
    def _backward(ctx, *grads):
        m, l, span = ctx.m, ctx.l, ctx.span
        B, I, Kq, p0, I_full, R = ctx.dims
        seed, rate = ctx.seed, ctx.rate
        cfg = m.config
        d, f, H = cfg.hidden_dim, cfg.ffn_dim, cfg.num_heads
        hd = d // H
        G = cfg.num_groups
        cached = span == 'N'
        written = ctx.state['written']
        acc = m.accumulate_grads or l in written
        written.add(l)
        mp = m.maps(B, I, max(Kq, 1), p0, I_full)
        tail = (Kq, I)
        dkv = None
        if Kq == 0:
            x, rstd1 = ctx.saved_tensors
            dev = x.device
            ma = mp['all'].to(dev)
            dqkv = grads[1].contiguous().clone()
            dqkv[:, :d].zero_()
            dx1 = None
        else:
            if cached:
                x, rstd1, qkv, o, lse, x1, rstd2, u, req_start, *rest = ctx.saved_tensors
                kv = rest[0] if rest else None
                dx2, dqkv_in = grads[0], None
            else:
                x, rstd1, qkv, o, lse, x1, rstd2, u = ctx.saved_tensors
                dx2, dqkv_in = grads
            dev = x.device
            ma, mt = mp['all'].to(dev), mp['tail'].to(dev)
            nt, nct = mp['tail'].ntiles, mp['tail'].chunks.shape[0]
            dx2 = dx2.contiguous()
            # FFN branch: dY2 = mask(dx2)
            if rate > 0:
                dy2 = torch.empty(B * Kq, d, device=dev)
                K.dropout_apply(dx2, d, dy2, d, B * Kq, d, seed, 2 * l + 1, rate, tail)
            else:
                dy2 = dx2
            K.wgrad(u, f, mt['rows'][1], dy2, d, mt['rows'][1], f, d, mt, nct, G, m.g(f'blk.{l}.w2'), f * d,
                    m.g(f'blk.{l}.b2'), d, a_xform=OT_AX_GELU, accumulate=acc, device=dev, m_rows=mp['tail'].nrows,
                    rowmap=mp['tail'])
            du = torch.empty(B * Kq, f, device=dev)
            K.gemm_rms(OT_GEMM_NT, dy2, d, d, mt['rows'][1], m.p(f'blk.{l}.w2'), f * d, d, f, mt['tile_group'], nt, du,
                       f, mt['rows'][1], epi=OT_EPI_GELU_BWD, aux=u, ldaux=f, m_rows=mp['tail'].nrows, device=dev)
            K.wgrad(x1, d, mt['rows'][1], du, f, mt['rows'][1], d, f, mt, nct, G, m.g(f'blk.{l}.w1'), d * f,
                    m.g(f'blk.{l}.b1'), f, a_xform=OT_AX_RMSNORM, rstd=rstd2, gamma=m.p(f'blk.{l}.norm2'),
                    accumulate=acc, device=dev, m_rows=mp['tail'].nrows, rowmap=mp['tail'])
            # FFN1 dgrad -> norm2 backward + residual; mask(dx1) for the attention branch
            dxn2 = torch.empty(B * Kq, d, device=dev)
            K.gemm_rms(OT_GEMM_NT, du, f, f, mt['rows'][1], m.p(f'blk.{l}.w1'), d * f, f, d, mt['tile_group'], nt,
                       dxn2, d, mt['rows'][1], epi=0, m_rows=mp['tail'].nrows, device=dev)
            dx1 = torch.empty(B * Kq, d, device=dev)
            dyo = torch.empty(B * Kq, d, device=dev) if rate > 0 else dx1
            K.rmsnorm_bwd(dxn2, d, x1, d, m.p(f'blk.{l}.norm2'), rstd2, dx1, d, B * Kq, d, dres=dx2, lddres=d,
                          dx_masked=dyo if rate > 0 else None, lddxm=d, seed=seed, site=2 * l, drop=rate, tail=tail,
                          dgamma=m.g(f'blk.{l}.norm2'), accumulate=acc, device=dev)
            _wgrad_single(m, o, dyo, d, d, mt, m.g(f'blk.{l}.wo'), acc, dev, mp['tail'].nrows, mp['tail'])
            do = torch.empty(B * Kq, d, device=dev)
            K.gemm_rms(OT_GEMM_NT, dyo, d, d, mt['rows'][1], m.p(f'blk.{l}.wo'), 0, d, d, mt['tile_group'], nt, do, d,
                       mt['rows'][1], epi=0, m_rows=mp['tail'].nrows, device=dev)
            # attention
            dqkv = torch.empty(B * I, 3 * d, device=dev)
            if Kq < I:
                dqkv[:, :d].zero_()
            if cached:
                Ic = kv.shape[0] // R if kv is not None else 0
                if kv is not None:
                    dkv = torch.zeros(R * Ic, 3 * d, device=dev)        # the S span's qkv gradient: dK | dV, dQ = 0
                K.attn_bwd_cached(qkv, 3 * d, (kv, d) if kv is not None else None, 3 * d, req_start, R, B, H, Ic, I,
                                  Kq, hd, o, do, lse, dqkv, (dkv, d) if dkv is not None else None)
            else:
                K.attn_bwd(qkv, 3 * d, o, do, lse, B, H, I, Kq, hd, dqkv)
                if dqkv_in is not None:
                    dqkv[:, d:] += dqkv_in[:, d:]                       # the N span's dK / dV of these rows
        nca = mp['all'].chunks.shape[0]
        K.wgrad(x, d, ma['rows'][0], dqkv, 3 * d, ma['rows'][0], d, 3 * d, ma, nca, G, m.g(f'blk.{l}.wqkv'),
                3 * d * d, None, 0, a_xform=OT_AX_RMSNORM, rstd=rstd1, gamma=m.p(f'blk.{l}.norm1'), accumulate=acc,
                device=dev, m_rows=mp['all'].nrows, rowmap=mp['all'])
        dxn1 = torch.empty(B * I, d, device=dev)
        K.gemm_rms(OT_GEMM_NT, dqkv, 3 * d, 3 * d, ma['rows'][0], m.p(f'blk.{l}.wqkv'), 3 * d * d, 3 * d, d,
                   ma['tile_group'], mp['all'].ntiles, dxn1, d, ma['rows'][0], epi=0, m_rows=mp['all'].nrows,
                   device=dev)
        dx = torch.empty(B * I, d, device=dev)
        K.rmsnorm_bwd(dxn1, d, x, d, m.p(f'blk.{l}.norm1'), rstd1, dx, d, B * I, d, dres=dx1, lddres=d,
                      dres_tail=(Kq, I) if 0 < Kq < I else (0, 0), dgamma=m.g(f'blk.{l}.norm1'), accumulate=acc,
                      device=dev)
        return (None, dx, dkv) + (None,) * 14


# =============================================================================== the model path
def forward_probs_requests(m, ns: Dict, seq: Dict, req, training: bool = False, validate: bool = True):
    """[T, C] probabilities (``_ot_logits`` set, like ``forward_probs``) of C candidates (``ns``, C rows) of R
    requests (``seq``, R rows), ``req`` [C] the request of each candidate."""
    check_supported(m)
    cfg = m.config
    d = cfg.hidden_dim
    if not ns or not seq:
        raise ValueError('forward_requests: both non-sequence features (per candidate) and sequence features '
                         '(per request) are needed')
    C = int(next(iter(ns.values())).shape[0])
    R = int(next(iter(seq.values())).shape[0])
    if validate:
        check_req('forward_requests', req, R, C, ordered=True)
    elif torch.as_tensor(req).numel() != C:
        raise ValueError(f'forward_requests: {torch.as_tensor(req).numel()} request indices for {C} candidates')
    if C == 0 or R == 0:
        raise ValueError('forward_requests: an empty batch')
    dev = m.device
    req = torch.as_tensor(req).to(dev, torch.int32).contiguous()
    req_start = torch.searchsorted(req, torch.arange(R + 1, device=dev, dtype=torch.int32)).to(torch.int32)
    plan_s = m._plan({}, seq, training)
    plan_n = m._plan(ns, {}, training)
    if plan_s['seq_map'] is None:
        raise ValueError('forward_requests: no configured sequence feature in seq_features')
    seed = 0
    if training:
        m._step += 1
        seed = (m.dropout_seed + 0x9E3779B9 * m._step) & 0xFFFFFFFF
    xs, xn = _TokenizeRequests.apply(m.flat, m, plan_s, plan_n)
    state = {'written': set()}
    for l, e in enumerate(request_schedule(cfg, plan_s['L_S'])):
        s, n, kS, kN, I_full = e['s'], e['n'], e['kS'], e['kN'], e['I']
        kv = None
        if s > 0:
            xs, kv = _SpanBlock.apply(m.flat, xs, None, m, l, 'S', R, s, kS, 0, I_full, layer_seed(seed, 0, s, d),
                                      training, None, None, R, state)
        xn = _SpanBlock.apply(m.flat, xn, kv, m, l, 'N', C, n, kN, s, I_full, n_span_seed(seed), training, req,
                              req_start, R, state)
    probs, logits = _Head.apply(m.flat, xn, m)
    probs._ot_logits = logits
    return probs
