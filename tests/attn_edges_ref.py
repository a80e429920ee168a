"""Attention on saturating and peaked softmax rows: the inputs, the float64 reference and the yardsticks (no GPU).

The kernel tests elsewhere draw q, k from randn, so every score q.k / sqrt(hd) lies in about [-5, 5]: a kernel that
forgot the running-max subtraction, rescaled wrongly when the maximum rises, took the maximum before the mask or lost
lse at large m would pass them.  The cases here put the scores where those mistakes are O(1):

  peaked            randn, q and k each x 6: score std ~ 36, rows near one-hot
  rising            c_j = 120 - 0.5 (J - 1 - j): the maximum at the newest visible key (every 32-key block raises the
                    running maximum by 16); the causally masked keys hold the largest scores
  falling           c_j = 120 - 0.5 j: the maximum in the first key block, later blocks contribute exact zeros
  all_negative      c_j = -130: a softmax as wide as randn's whose every exp(s) underflows without the subtraction
  dominant_invalid  (masked entry points) invalid keys c_j = +120, valid keys c_j = 0

built as q_i = w + noise_i (noise orthogonal to w, w.w / sqrt(hd) = 1 per (sample, head)) and k_j = c_j w + randn, so
score(i, j) = c_j + N(0, ~1) and the offset is not multiplied by noise.  j is the absolute key position (cached
layouts: over [cache rows | own rows], w per (request, head)).  Every value is a float64 that float32 holds exactly.

Reference: float64, -inf masking, logsumexp, autograd.  One function (``attend``) over the expanded problem
(queries [N, Kq], keys [N, J], a visibility mask [N, Kq, J]); ``plain`` and ``cached`` build that problem from the
plain / selected-query / masked and the cached / masked-cache / bf16-cache layouts.  tests/request_attn_ref.py and
tests/kv16_ref.py state the cached operations themselves; tests/test_attn_edges_ref.py checks this file against them.

Yardsticks: the error of the same function evaluated in float32 on the CPU (``e32``), per output, for the f32-accurate
kernels — for the gradients of the f32-arithmetic backwards the larger of that and of the recomputing algorithm's
float32 evaluation (``evaluate_recompute``); for the bf16 mode the error of a float64 evaluation that rounds where
the kernels of attention_bf16.hip round (``bf16_emulation``).  A kernel passes when
max |kernel - f64| <= margin * yardstick + 8 * 2^-24 * max |f64|.
"""

import functools
import math

import torch

CASES = ('peaked', 'rising', 'falling', 'all_negative')
PEAK = 120.0            # the dominant offset of rising / falling / dominant_invalid
FLOOR_ULPS = 8          # the floor of tests/test_pair_precision_gpu.py::check_ratio

# margins over the yardstick, set before any GPU run (profiles/r19/attn_softmax_edges.md has the reasoning)
MARGIN_F32 = 8          # f32-arithmetic kernels: the project's 4 ("as accurate as f32") x 2 (sequential MFMA sums)
MARGIN_PAIR = 32        # two-plane fp16 pair: 22 significand bits against 24, x 4
MARGIN_BF16 = 4         # bf16 mode, over the bf16 emulation


def _f32_exact(x):
    return x.float().double()


def offsets(case, J, valid=None):
    """c_j [J] (or [N, J] under ``valid``) of a structured case."""
    j = torch.arange(J, dtype=torch.float64)
    if case == 'rising':
        return PEAK - 0.5 * (J - 1 - j)
    if case == 'falling':
        return PEAK - 0.5 * j
    if case == 'all_negative':
        return torch.full((J,), -130.0, dtype=torch.float64)
    if case == 'dominant_invalid':
        return torch.where(torch.as_tensor(valid, dtype=torch.bool), 0.0, PEAK).double()
    raise ValueError(case)


def _directions(N, H, hd, g):
    w = torch.randn(N, H, hd, generator=g, dtype=torch.float64)
    return w * math.sqrt(math.sqrt(hd)) / w.norm(dim=-1, keepdim=True)             # w.w = sqrt(hd)


def _structured(case, w, qn, kn, c):
    """w [N, H, hd]; qn, kn [N, J, H, hd] randn; c [J] or [N, J] -> q = w + noise (noise orthogonal to w), k = c w + kn."""
    ww = (w * w).sum(-1)                                                            # [N, H]
    q = w[:, None] + qn - ((qn * w[:, None]).sum(-1) / ww[:, None])[..., None] * w[:, None]
    c = c if c.dim() == 2 else c[None]
    return q, c[:, :, None, None] * w[:, None] + kn


def make(case, B, H, I, hd, seed, valid=None):
    """qkv [B*I, 3d] float64 (float32-exact).  ``valid`` [B, I] (bool): the key-padding mask of 'dominant_invalid'."""
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    q, k, v = (torch.randn(B, I, H, hd, generator=g, dtype=torch.float64) for _ in range(3))
    if case == 'peaked':
        q, k = 6.0 * q, 6.0 * k
    elif case != 'randn':               # 'randn': what the other kernel tests draw (the self-checks' baseline)
        q, k = _structured(case, _directions(B, H, hd, g), q, k, offsets(case, I, valid))
    return _f32_exact(torch.cat([q.reshape(B * I, d), k.reshape(B * I, d), v.reshape(B * I, d)], 1))


def make_dout(rows, d, seed):
    g = torch.Generator().manual_seed(seed + 77)
    return _f32_exact(torch.randn(rows, d, generator=g, dtype=torch.float64))


def make_valid(B, I, seed):
    """bool [B, I], about 70% ones; key 0 invalid (a query that sees only itself), the last key valid."""
    g = torch.Generator().manual_seed(seed + 13)
    valid = torch.rand(B, I, generator=g) < 0.7
    valid[:, 0] = False
    valid[:, -1] = True
    return valid


def make_cached(case, cands, H, Ic, n, hd, seed, cache_valid=None):
    """Request r has cands[r] candidates of n own rows over Ic cached rows.  Returns (qkv [C*n, 3d], kv [R*Ic, 2d],
    req [C]); key j of a candidate's sequence is cached row j (< Ic) or own row j - Ic; ``cache_valid`` [R, Ic]."""
    g = torch.Generator().manual_seed(seed)
    R, C, d, J = len(cands), sum(cands), H * hd, Ic + n
    req = torch.repeat_interleave(torch.arange(R), torch.tensor(cands))
    q, k, v = (torch.randn(C, n, H, hd, generator=g, dtype=torch.float64) for _ in range(3))
    kc, vc = (torch.randn(R, Ic, H, hd, generator=g, dtype=torch.float64) for _ in range(2))
    if case == 'peaked':
        q, k, kc = 6.0 * q, 6.0 * k, 6.0 * kc
    else:
        w = _directions(R, H, hd, g)
        if case == 'dominant_invalid':
            c = offsets(case, J, torch.cat([torch.as_tensor(cache_valid, dtype=torch.bool)[:, :Ic],
                                            torch.ones(R, n, dtype=torch.bool)], 1))                 # [R, J]
        else:
            c = offsets(case, J)[None].expand(R, J)
        q, k = _structured(case, w[req], q, k, c[req][:, Ic:])
        kc = c[:, :Ic, None, None] * w[:, None] + kc
    qkv = torch.cat([q.reshape(C * n, d), k.reshape(C * n, d), v.reshape(C * n, d)], 1)
    kv = torch.cat([kc.reshape(R * Ic, d), vc.reshape(R * Ic, d)], 1)
    return _f32_exact(qkv), _f32_exact(kv), req


# ------------------------------------------------------------------------------------------------ the operation
def attend(q, k, v, vis):
    """q [N, Kq, H, hd], k / v [N, J, H, hd], vis [N, Kq, J] (bool) -> out [N, Kq, H*hd], lse [N, H, Kq], in the
    operands' dtype: s = q.k / sqrt(hd), -inf where not visible, lse = logsumexp, out = exp(s - lse) v."""
    N, Kq, H, hd = q.shape
    s = torch.einsum('nqhe,nkhe->nhqk', q, k) / math.sqrt(hd)
    s = s.masked_fill(~vis[:, None], float('-inf'))
    lse = torch.logsumexp(s, -1)
    out = torch.einsum('nhqk,nkhe->nqhe', torch.exp(s - lse[..., None]), v)
    return out.reshape(N, Kq, H * hd), lse


def scores(q, k, vis):
    """Float64 scores [N, H, Kq, J] and the visibility broadcast to them."""
    s = torch.einsum('nqhe,nkhe->nhqk', q.double(), k.double()) / math.sqrt(q.shape[-1])
    return s, vis[:, None].expand_as(s)


def visibility(qpos, J, valid=None):
    """qpos [N, Kq] -> [N, Kq, J]: key j <= the query's position, and under ``valid`` [N, J] (valid j or j == position)
    — the rule of attn.h."""
    kpos = torch.arange(J)[None, None, :]
    vis = kpos <= qpos[:, :, None]
    if valid is not None:
        vis = vis & (torch.as_tensor(valid, dtype=torch.bool)[:, None, :] | (kpos == qpos[:, :, None]))
    return vis


def tail_qpos(B, I, Kq):
    return torch.arange(I - Kq, I)[None].expand(B, Kq)


def plain(qkv, B, H, I, hd, qpos, valid=None):
    """The plain / selected-query / masked layout (attn.h): qkv [B*I, 3d], queries at qpos [B, Kq]."""
    d = H * hd
    x = qkv[:, :3 * d].reshape(B, I, 3, H, hd)
    q = x[:, :, 0][torch.arange(B)[:, None], qpos]
    return q, x[:, :, 1], x[:, :, 2], visibility(qpos, I, valid)


def cached(qkv, kv, req, H, Ic, n, Kq, hd, cache_valid=None):
    """The cached layouts: candidate c's keys are its request's Ic cached rows (kv [R*Ic, 2d]: k | v) then its own n
    rows (qkv [C*n, 3d]); its last Kq rows are the queries, at positions Ic + n - Kq + j; ``cache_valid`` [R, Ic]
    masks cached rows (own rows are valid)."""
    d = H * hd
    C, R = qkv.shape[0] // n, kv.shape[0] // max(Ic, 1)
    x = qkv[:, :3 * d].reshape(C, n, 3, H, hd)
    c = kv[:, :2 * d].reshape(R, Ic, 2, H, hd)
    k = torch.cat([c[req][:, :, 0], x[:, :, 1]], 1)
    v = torch.cat([c[req][:, :, 1], x[:, :, 2]], 1)
    valid = None
    if cache_valid is not None:
        valid = torch.cat([torch.as_tensor(cache_valid, dtype=torch.bool)[req][:, :Ic],
                           torch.ones(C, n, dtype=torch.bool)], 1)
    return x[:, n - Kq:, 0], k, v, visibility(tail_qpos(C, Ic + n, Kq), Ic + n, valid)


def evaluate(layout, leaves, dout, dtype=torch.float64):
    """layout(*leaves) -> (q, k, v, vis).  Runs ``attend`` and its autograd gradient in ``dtype``; returns float64
    {'out' [N*Kq, d], 'lse' [N, H, Kq], 'grads': one tensor per leaf}."""
    xs = [x.to(dtype).clone().requires_grad_(True) for x in leaves]
    out, lse = attend(*layout(*xs))
    out = out.reshape(-1, out.shape[-1])
    (out * dout.to(dtype)).sum().backward()
    return {'out': out.detach().double(), 'lse': lse.detach().double(),
            'grads': [(x.grad if x.grad is not None else torch.zeros_like(x)).double() for x in xs]}


def evaluate_recompute(layout, leaves, dout, dtype=torch.float32):
    """The same operation by the algorithm every backward kernel here implements, in ``dtype`` on the CPU: an
    online-softmax forward in log2 units (q x log2(e) / sqrt(hd) folded, lse = m ln2 + log(l), O and lse kept in
    ``dtype``) and a backward that RECOMPUTES P = exp(q.k / sqrt(hd) - lse) from the stored lse and takes
    delta = rowsum(dO . O) from the stored O, dS = P (dP - delta) / sqrt(hd).

    ``evaluate``'s autograd keeps the forward's P, so on a one-hot row it cancels exactly (P = exp(0) = 1,
    dP - sum_j P_j dP_j = 0) what no recomputing backward can: lse is stored with a rounding of its own at the scores'
    magnitude (2^-24 x 120 = 7e-6, relative, on every P of the row) and delta is another dot product than dP.  The
    f32-arithmetic backward kernels are held to the larger of the two evaluations' errors
    (profiles/r19/attn_softmax_edges.md).  Returns {'out', 'lse', 'grads'} like ``evaluate``."""
    xs = [x.to(dtype).clone().requires_grad_(True) for x in leaves]
    q, k, v, vis = layout(*xs)
    N, Kq, H, hd = q.shape
    hide = ~vis[:, None]
    with torch.no_grad():
        scale = torch.tensor(1.0 / math.sqrt(hd), dtype=dtype)
        qscale = scale * torch.tensor(1.4426950408889634, dtype=dtype)
        s2 = torch.einsum('nqhe,nkhe->nhqk', q * qscale, k).masked_fill(hide, float('-inf'))
        m = s2.max(-1, keepdim=True).values
        e = torch.exp2(s2 - m)
        l = e.sum(-1, keepdim=True)
        out = torch.einsum('nhqk,nkhe->nqhe', e, v) / l.permute(0, 2, 1, 3)
        lse = m * torch.tensor(math.log(2.0), dtype=dtype) + torch.log(l)                  # [N, H, Kq, 1]
        do = dout.to(dtype).reshape(N, Kq, H, hd)
        P = torch.exp(torch.einsum('nqhe,nkhe->nhqk', q, k) * scale - lse).masked_fill(hide, 0.0)
        delta = (do * out).sum(-1).permute(0, 2, 1)[..., None]
        dS = P * (torch.einsum('nqhe,nkhe->nhqk', do, v) - delta) * scale
        dv = torch.einsum('nhqk,nqhe->nkhe', P, do)
        dk = torch.einsum('nhqk,nqhe->nkhe', dS, q)
        dq = torch.einsum('nhqk,nkhe->nqhe', dS, k)
    grads = torch.autograd.grad([q, k, v], xs, [dq, dk, dv], allow_unused=True)          # the layout's transpose
    return {'out': out.reshape(N * Kq, H * hd).double(), 'lse': lse[..., 0].double(),
            'grads': [(g if g is not None else torch.zeros_like(x)).double() for g, x in zip(grads, xs)]}


def split_dqkv(g, d):
    """dqkv [rows, 3d] -> {'dq', 'dk', 'dv'}: their scales differ, so each is bounded on its own."""
    return {'dq': g[:, :d], 'dk': g[:, d:2 * d], 'dv': g[:, 2 * d:3 * d]}


# ------------------------------------------------------------------------------------------------ the bf16 mode
def bf16(x):
    """Round to bf16 (nearest even) and back to float64."""
    return x.float().to(torch.bfloat16).double()


def bf16_emulation(qkv, dout, B, H, I, hd, qpos, planes_fwd=True, planes_bwd=True):
    """Float64 arithmetic with the roundings of the bf16-mode kernels (attention_bf16.hip), on operands that are bf16
    values already (rounding q, k, v, dO is then the identity).

    Forward, one plane (attn_fwd_split_kernel<HD, 1>): q x (log2(e) / sqrt(hd)), the product formed in f32, is rounded
    to bf16 before S — a rounding of its own even for a bf16 q; P = exp2(s - m) is rounded for P V while l sums the
    unrounded values; lse = m ln2 + log(l).  Backward (attn_bwd_split_kernel<HD, 1>, attn_bwd_group_kernel): S from
    the plain operands, P = exp(s / sqrt(hd) - lse) with the FORWARD's lse and delta = rowsum(dO . O) with the forward's
    O; P rounded for dV, dS = P (dP - delta) / sqrt(hd) (from the unrounded P) rounded for dK and dQ.
    ``planes_bwd`` False: a backward in f32 arithmetic behind the one-plane forward (the short-tail backward in bf16
    mode) — the forward's O and lse, no rounding of P / dS.  Returns {'out', 'lse', 'grads': [dqkv]} like evaluate."""
    d = H * hd
    q, k, v, vis = plain(qkv.double(), B, H, I, hd, qpos)
    Kq = qpos.shape[1]
    m4 = ~vis[:, None]
    if planes_fwd:
        qscale = torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32) * torch.tensor(1.4426950408889634,
                                                                                       dtype=torch.float32)
        q2 = (q.float() * qscale).to(torch.bfloat16).double()
        s2 = torch.einsum('nqhe,nkhe->nhqk', q2, k).masked_fill(m4, float('-inf'))           # log2 units
        m = s2.max(-1, keepdim=True).values
        e = torch.exp2(s2 - m)
        l = e.sum(-1, keepdim=True)
        out = torch.einsum('nhqk,nkhe->nqhe', bf16(e) / l, v).reshape(B, Kq, d)
        lse = (m * math.log(2.0) + torch.log(l))[..., 0]
    else:
        out, lse = attend(q, k, v, vis)
    s = torch.einsum('nqhe,nkhe->nhqk', q, k) / math.sqrt(hd)
    P = torch.exp(s - lse[..., None]).masked_fill(m4, 0.0)
    do = dout.double().reshape(B, Kq, H, hd)
    delta = (do * out.reshape(B, Kq, H, hd)).sum(-1).permute(0, 2, 1)                         # [B, H, Kq]
    dP = torch.einsum('nqhe,nkhe->nhqk', do, v)
    dS = P * (dP - delta[..., None]) / math.sqrt(hd)
    Pr, dSr = (bf16(P), bf16(dS)) if planes_bwd else (P, dS)
    dv = torch.einsum('nhqk,nqhe->nkhe', Pr, do).reshape(B, I, d)
    dk = torch.einsum('nhqk,nqhe->nkhe', dSr, q).reshape(B, I, d)
    dq_rows = torch.einsum('nhqk,nkhe->nqhe', dSr, k).reshape(B, Kq, d)
    dq = torch.zeros(B, I, d, dtype=torch.float64)
    dq[torch.arange(B)[:, None], qpos] = dq_rows
    return {'out': out.reshape(B * Kq, d), 'lse': lse,
            'grads': [torch.cat([dq, dk, dv], -1).reshape(B * I, 3 * d)]}


# ------------------------------------------------------------------------------------------------ the bound
def err(got, ref):
    return (got.double() - ref).abs().max().item()


def bound(e_yard, ref, margin):
    return margin * e_yard + FLOOR_ULPS * 2.0 ** -24 * ref.abs().max().item()


def within(got, ref, e_yard, margin):
    """Finite everywhere and max |got - ref| <= margin * e_yard + the floor."""
    return bool(torch.isfinite(got).all()) and err(got, ref) <= bound(e_yard, ref, margin)


# ------------------------------------------------------------------------------------------------ the problems
def select_qpos(B, I, Kq, seed):
    """Kept query positions as ot_pyramid_select gives them: ascending, the last token always kept."""
    g = torch.Generator().manual_seed(seed + 5)
    return torch.stack([torch.cat([torch.sort(torch.randperm(I - 1, generator=g)[:Kq - 1]).values,
                                   torch.tensor([I - 1])]) for _ in range(B)])


def visible_max(qkv, B, H, I, hd, qpos, valid=None):
    q, k, _, vis = plain(qkv, B, H, I, hd, qpos, valid)
    s, see = scores(q, k, vis)
    return s[see].max().item()


@functools.lru_cache(maxsize=None)
def plain_problem(case, B, H, I, Kq, hd, sel=False, masked=False, operands_bf16=False):
    """One problem per (case, shape), shared by the CPU and the GPU tests: operands, the float64 reference and the
    float32 yardstick.  'peaked' draws 36 x N(0, 1) scores, whose maximum over a small problem is not always past
    100: the seed is the first of seed0, seed0 + 1, .. whose visible maximum lies in [100, 200] (the property
    tests/test_attn_edges_ref.py asserts), fixed before any kernel sees the data.  ``operands_bf16``: qkv and dout
    rounded to bf16 (the bf16 mode's reference)."""
    seed0 = 1000 * I + 10 * Kq + hd + B
    qpos = select_qpos(B, I, Kq, seed0) if sel else tail_qpos(B, I, Kq)
    valid = make_valid(B, I, seed0) if masked else None
    for seed in range(seed0, seed0 + 200):
        qkv = make(case, B, H, I, hd, seed, valid)
        if operands_bf16:
            qkv = bf16(qkv)
        if case != 'peaked' or 100.0 <= visible_max(qkv, B, H, I, hd, qpos, valid) <= 200.0:
            break
    else:
        raise AssertionError(f'no peaked seed at {(B, H, I, Kq, hd)}')
    dout = make_dout(B * Kq, H * hd, seed)
    if operands_bf16:
        dout = bf16(dout)
    layout = lambda x: plain(x, B, H, I, hd, qpos, valid)
    ref = evaluate(layout, [qkv], dout)
    f32 = evaluate(layout, [qkv], dout, torch.float32)
    rec32 = evaluate_recompute(layout, [qkv], dout)
    return {'qkv': qkv, 'dout': dout, 'qpos': qpos, 'valid': valid, 'layout': layout, 'ref': ref, 'f32': f32,
            'rec32': rec32}


@functools.lru_cache(maxsize=None)
def cached_problem(case, cands, H, Ic, n, Kq, hd, masked=False, cache_bf16=False):
    """As plain_problem for the cached layouts; ``cache_bf16``: the cache rounded to bf16 (the kv16 entry point: the
    reference runs on the rounded cache)."""
    seed0 = 1000 * Ic + 10 * n + Kq + hd
    R = len(cands)
    cv = make_valid(R, Ic, seed0) if masked else None
    for seed in range(seed0, seed0 + 200):
        qkv, kv, req = make_cached(case, list(cands), H, Ic, n, hd, seed, cv)
        if cache_bf16:
            kv = bf16(kv)
        layout = lambda x, c: cached(x, c, req, H, Ic, n, Kq, hd, cv)
        if case == 'peaked':
            q, k, _, vis = layout(qkv, kv)
            s, see = scores(q, k, vis)
            if not 100.0 <= s[see].max().item() <= 200.0:
                continue
        break
    else:
        raise AssertionError(f'no peaked seed at {(cands, H, Ic, n, Kq, hd)}')
    dout = make_dout(sum(cands) * Kq, H * hd, seed)
    ref = evaluate(layout, [qkv, kv], dout)
    f32 = evaluate(layout, [qkv, kv], dout, torch.float32)
    rec32 = evaluate_recompute(layout, [qkv, kv], dout)
    return {'qkv': qkv, 'kv': kv, 'req': req, 'dout': dout, 'cache_valid': cv, 'layout': layout, 'ref': ref,
            'f32': f32, 'rec32': rec32}


# ------------------------------------------------------------------------------------------------ the GPU file's shapes
# (route, matmul mode, (B, H, I, Kq, hd), selected queries): the smallest shapes of the existing tests that reach each
# route; tests/test_attn_softmax_edges_gpu.py runs them, tests/test_attn_edges_ref.py proves the cases on them
FWD = ([('TAIL', 'f32', s, False) for s in [(2, 2, 70, 4, 64), (1, 2, 40, 1, 32), (1, 1, 33, 2, 128)]]
       + [('SHARED_KV', 'f32', s, False) for s in [(2, 4, 100, 96, 32), (1, 2, 100, 96, 64), (3, 4, 130, 70, 16)]]
       + [('WAVE', 'f32', s, False) for s in [(2, 2, 150, 150, 64), (1, 2, 33, 17, 128), (3, 4, 40, 12, 16)]]
       + [('SLICE', 'split', s, False) for s in [(2, 4, 140, 140, 32), (2, 2, 144, 144, 64), (2, 2, 100, 37, 64)]]
       + [('SLICE', 'split', (2, 4, 140, 70, 32), True)]
       + [('PLANES3', 'split', s, False) for s in [(2, 4, 300, 300, 32), (1, 2, 300, 137, 64), (1, 2, 290, 100, 128)]]
       + [('PLANES1', 'bf16', s, False) for s in [(2, 2, 150, 150, 64), (2, 4, 40, 12, 32)]])

BWD = ([('SLICE', 'split', s, False) for s in [(2, 4, 140, 140, 32), (2, 2, 144, 144, 64), (2, 2, 161, 150, 64),
                                               (2, 2, 289, 100, 64), (2, 2, 544, 272, 64)]]
       + [('FDL', 'f32', (2, 4, 170, 160, 32), False), ('FDL', 'split', (2, 4, 260, 77, 32), False)]
       + [('TAIL', m, s, False) for s in [(2, 4, 140, 3, 32), (2, 2, 70, 4, 64), (3, 4, 40, 1, 16)]
          for m in ('f32', 'split')]
       + [('TAIL', 'bf16', (2, 4, 140, 3, 32), False)]
       + [('WAVE', 'f32', s, False) for s in [(1, 4, 170, 161, 32), (2, 2, 70, 33, 64)]]
       + [('WAVE', m, s, False) for s in [(1, 2, 33, 17, 128), (3, 4, 40, 12, 16)] for m in ('f32', 'split')]
       + [('WAVE', m, (2, 4, 140, 70, 32), True) for m in ('f32', 'split')]
       + [('KGROUP', 'bf16', s, False) for s in [(2, 2, 300, 300, 64), (2, 4, 260, 77, 32)]]
       + [('BF16', 'bf16', (2, 2, 150, 150, 64), False), ('BF16', 'bf16', (2, 2, 300, 120, 64), True)])

# masked entry points: one TAIL and one WAVE shape per head_dim (tests/test_padding_mask_gpu.py's B, H, I, Kq)
MASKED = [(3, 2, I, Kq, hd) for hd in (16, 32, 64, 128) for I, Kq in ((37, 3), (70, 70))]
MASKED_CASES = ('rising', 'dominant_invalid')

CANDS = (3, 0, 9, 1, 40)            # tests/test_request_attn_gpu.py's: an empty request, query counts across 32 and 64
CACHED = [(2, hd, Ic, n, Kq) for hd in (32, 64) for Ic in (33, 70) for n, Kq in ((12, 7), (33, 33))]
CACHED_MASKED = ((2, 0, 1, 2), 2, 32, 40, 4, 4)       # (cands, H, hd, Ic, n, Kq): test_masked_cached_attention's sizes
KV16 = [((2, 0, 1, 2), 2, hd, 40, 4, 4) for hd in (32, 64)]


def entry_id(e):
    route, mode, shape, sel = e
    return f'{route}-{mode}-' + '-'.join(map(str, shape)) + ('-sel' if sel else '')
