"""float64 yardstick for the cached attention of request-grouped training (no GPU).

Candidate c of request req[c] attends with the last Kq of its n rows over the request's Ic cached
K/V rows and its own n rows; query j sits at absolute position Ic + n - Kq + j.  The reference
works on the *expanded* problem: each candidate's keys are the concatenation of its request's cached
rows and its own rows under the plain causal mask, and the gradients come from autograd, so a cached
row's dK/dV is the sum over the request's candidates by construction."""

import math

import torch


def forward(q, k, v, kc, vc, req, H, Kq):
    """q, k, v: [C, n, d]; kc, vc: [R, Ic, d]; req: [C] -> out [C, Kq, d], lse [C, H, Kq] (float64)."""
    C, n, d = q.shape
    Ic, hd = kc.shape[1], d // H
    req = torch.as_tensor(req, dtype=torch.long)
    keys = torch.cat([kc[req], k], 1).reshape(C, Ic + n, H, hd)          # the expanded batch's keys
    vals = torch.cat([vc[req], v], 1).reshape(C, Ic + n, H, hd)
    qs = q[:, n - Kq:].reshape(C, Kq, H, hd)
    s = torch.einsum('cqhe,ckhe->chqk', qs, keys) / math.sqrt(hd)
    qpos = Ic + n - Kq + torch.arange(Kq)
    mask = torch.arange(Ic + n)[None, :] <= qpos[:, None]                # [Kq, Ic + n]
    s = s.masked_fill(~mask, float('-inf'))
    lse = torch.logsumexp(s, -1)                                         # [C, H, Kq]
    p = torch.exp(s - lse[..., None])
    out = torch.einsum('chqk,ckhe->cqhe', p, vals).reshape(C, Kq, d)
    return out, lse


def forward_backward(qkv, kv, req, R, H, Ic, n, Kq, dout):
    """qkv [C*n, >= 3d] (q | k | v), kv [R*Ic, >= 2d] (k | v), dout [C*Kq, d]; any float dtype.
    Returns float64 out [C*Kq, d], lse [C, H, Kq], dqkv [C*n, 3d] (dq of the rows without a query is 0),
    dkv [R*Ic, 2d] (summed over each request's candidates)."""
    d = dout.shape[1]
    C = qkv.shape[0] // n
    x = qkv[:, :3 * d].double().reshape(C, n, 3 * d).clone().requires_grad_(True)
    c = kv[:, :2 * d].double().reshape(R, Ic, 2 * d).clone().requires_grad_(True)
    out, lse = forward(x[..., :d], x[..., d:2 * d], x[..., 2 * d:], c[..., :d], c[..., d:], req, H, Kq)
    (out.reshape(C * Kq, d) * dout.double()).sum().backward()
    dx = x.grad if x.grad is not None else torch.zeros_like(x)
    dc = c.grad if c.grad is not None else torch.zeros_like(c)
    return (out.detach().reshape(C * Kq, d), lse.detach(), dx.reshape(C * n, 3 * d), dc.reshape(R * Ic, 2 * d))


def per_candidate_dkv(qkv, kv, req, R, H, Ic, n, Kq, dout):
    """The cached rows' gradient of every candidate taken alone: [C, Ic, 2d] (self-test of the sum)."""
    d = dout.shape[1]
    C = qkv.shape[0] // n
    parts = []
    for ci in range(C):
        one = kv[:, :2 * d].double().reshape(R, Ic, 2 * d)[int(req[ci])][None]
        _, _, _, dc = forward_backward(qkv[ci * n:(ci + 1) * n], one.reshape(Ic, 2 * d), [0], 1, H, Ic, n, Kq,
                                       dout[ci * Kq:(ci + 1) * Kq])
        parts.append(dc.reshape(Ic, 2 * d))
    return torch.stack(parts) if parts else torch.zeros(0, Ic, 2 * d, dtype=torch.float64)
