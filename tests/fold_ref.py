"""Float64 reference of the folded one-query attention (recommend_amd/csrc/attention_fold.hip) and of
the unfolded attention it must equal.

One layer, one query per sample (the last position, which sees every key).  S = the key positions of weight group 0
(shared), D = the positions of the dedicated groups.  xh_j = x_j rstd_j; gamma = norm1's weight; Wk0 / Wv0 [d, d] =
group 0's K / V blocks; q [B, d] = the query (an input here: the model's tail GEMM forms it); Kd / Vd [B, |D|, d] = the
projected rows of the dedicated keys.

``fold_forward`` / ``fold_backward`` are the formulas the kernels implement; ``unfolded`` projects K / V for every shared
row, runs softmax and PV, and takes the gradients by autograd."""

import math

import torch


def rstd_of(x, eps=1e-6):
    return torch.rsqrt((x * x).mean(-1) + eps)


def fold_forward(xh, gamma, Wk0, Wv0, q, Kd, Vd, S, D, H):
    """-> dict(o [B, d], lse [B, H], y [B, H, d], p [B, H, I], a [B, H, d], qt [B, H, d])."""
    B, I, d = xh.shape
    hd = d // H
    qh = q.reshape(B, H, hd)
    a = torch.einsum('khc,bhc->bhk', Wk0.reshape(d, H, hd), qh)
    qt = gamma * a
    s = xh.new_zeros(B, H, I)
    s[:, :, S] = torch.einsum('bjk,bhk->bhj', xh[:, S], qt) / math.sqrt(hd)
    s[:, :, D] = torch.einsum('bjhc,bhc->bhj', Kd.reshape(B, len(D), H, hd), qh) / math.sqrt(hd)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    y = torch.einsum('bhj,bjk->bhk', p[:, :, S], xh[:, S])
    o = torch.einsum('khc,bhk->bhc', Wv0.reshape(d, H, hd), gamma * y)
    o = o + torch.einsum('bhj,bjhc->bhc', p[:, :, D], Vd.reshape(B, len(D), H, hd))
    return dict(o=o.reshape(B, d), lse=lse, y=y, p=p, a=a, qt=qt)


def fold_backward(xh, rstd, gamma, Wk0, Wv0, q, Kd, Vd, S, D, H, fwd, do):
    """Given do [B, d] and ``fwd`` = fold_forward's dict -> dict(dx [B, I, d] (S rows; D rows zero), dq [B, d],
    dKd / dVd [B, |D|, d], dWk0 / dWv0 [d, d], dgamma [d], z [B, H, d], dgpart [B, d])."""
    B, I, d = xh.shape
    hd = d // H
    qh, doh = q.reshape(B, H, hd), do.reshape(B, H, hd)
    Wk, Wv = Wk0.reshape(d, H, hd), Wv0.reshape(d, H, hd)
    p, y, a, qt = fwd['p'], fwd['y'], fwd['a'], fwd['qt']
    b = torch.einsum('khc,bhc->bhk', Wv, doh)
    c = gamma * b
    delta = (fwd['o'].reshape(B, H, hd) * doh).sum(-1)
    dp = xh.new_zeros(B, H, I)
    dp[:, :, S] = torch.einsum('bjk,bhk->bhj', xh[:, S], c)
    dp[:, :, D] = torch.einsum('bjhc,bhc->bhj', Vd.reshape(B, len(D), H, hd), doh)
    ds = p * (dp - delta[..., None]) / math.sqrt(hd)
    z = torch.einsum('bhj,bjk->bhk', ds[:, :, S], xh[:, S])
    dq = torch.einsum('khc,bhk->bhc', Wk, gamma * z)
    dq = dq + torch.einsum('bhj,bjhc->bhc', ds[:, :, D], Kd.reshape(B, len(D), H, hd))
    dKd = torch.einsum('bhj,bhc->bjhc', ds[:, :, D], qh).reshape(B, len(D), d)
    dVd = torch.einsum('bhj,bhc->bjhc', p[:, :, D], doh).reshape(B, len(D), d)
    g = torch.einsum('bhj,bhk->bjk', ds[:, :, S], qt) + torch.einsum('bhj,bhk->bjk', p[:, :, S], c)
    xs = xh[:, S]
    dx = xh.new_zeros(B, I, d)
    dx[:, S] = rstd[:, S, None] * (g - xs * (g * xs).sum(-1, keepdim=True) / d)
    dWk0 = torch.einsum('bhk,bhc->khc', gamma * z, qh).reshape(d, d)
    dWv0 = torch.einsum('bhk,bhc->khc', gamma * y, doh).reshape(d, d)
    dgpart = (z * a + y * b).sum(1)
    return dict(dx=dx, dq=dq.reshape(B, d), dKd=dKd, dVd=dVd, dWk0=dWk0, dWv0=dWv0, dgamma=dgpart.sum(0), z=z,
                dgpart=dgpart)


def unfolded(x, gamma, Wk0, Wv0, q, Kd, Vd, S, D, H, do):
    """The same attention with K / V projected for every shared row, gradients by autograd: dict(o, lse, dx (S rows),
    dq, dKd, dVd, dWk0, dWv0, dgamma)."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, gamma, Wk0, Wv0, q, Kd, Vd)]
    x_, g_, Wk_, Wv_, q_, Kd_, Vd_ = leaves
    B, I, d = x.shape
    hd = d // H
    xn = x_ * rstd_of(x_)[..., None] * g_
    Kall, Vall = x.new_zeros(B, I, d), x.new_zeros(B, I, d)
    Kall[:, S], Vall[:, S] = xn[:, S] @ Wk_, xn[:, S] @ Wv_
    Kall[:, D], Vall[:, D] = Kd_, Vd_
    s = torch.einsum('bjhc,bhc->bhj', Kall.reshape(B, I, H, hd), q_.reshape(B, H, hd)) / math.sqrt(hd)
    p = torch.softmax(s, -1)
    o = torch.einsum('bhj,bjhc->bhc', p, Vall.reshape(B, I, H, hd)).reshape(B, d)
    (o * do).sum().backward()
    return dict(o=o.detach(), lse=torch.logsumexp(s.detach(), -1), dx=x_.grad, dq=q_.grad, dKd=Kd_.grad, dVd=Vd_.grad,
                dWk0=Wk_.grad, dWv0=Wv_.grad, dgamma=g_.grad)


def make_case(B, I, H, hd, ded, seed, dtype=torch.float64):
    """Seeded operands: ded = (first, end) of the dedicated positions.  Returns a dict of float64 tensors."""
    d = H * hd
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    D = list(range(ded[0], ded[1]))
    S = [j for j in range(I) if j not in D]
    x = rn(B, I, d) * 10.0 ** (-torch.rand(B, I, 1, generator=gen, dtype=torch.float64))   # rows of different size
    c = dict(x=x, gamma=1 + 0.1 * rn(d), Wk0=rn(d, d) / math.sqrt(d), Wv0=rn(d, d) / math.sqrt(d), q=rn(B, d),
             Kd=rn(B, len(D), d), Vd=rn(B, len(D), d), do=rn(B, d), dx1=rn(B, d), S=S, D=D, H=H)
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
