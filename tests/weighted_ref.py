"""The yardstick of the weighted-loss tests, in float64 numpy / torch, independent of
``recommend_amd``: the weighted task loss and its gradients (kernel level, and model level on
``oracle.onetrans_ref.forward``), the state ``ot_metrics_update_weighted`` accumulates, and Keras's weighted metrics
straight from the samples."""

import numpy as np
import torch

from oracle import onetrans_ref as R

EPS = 1e-7
W_MAX = 65536.0
UNIT = 1 << 24


def clamp_weights(w):
    """The kernels' reading of a weight: NaN and negatives 0, above the range its end."""
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.where(w > 0, np.minimum(w, W_MAX), 0.0)


def units(w):
    """Metric units of f32 weights: clamp, then the nearest multiple of 2^-24 (ties to even), as int64."""
    return np.rint(clamp_weights(w) * UNIT).astype(np.int64)


def _terms(y, p, z, mse, prob_form):
    """[T, B] per-element terms (torch float64) with the zero-weight entries already made finite by the caller."""
    rows = []
    for t in range(y.shape[0]):
        if mse[t]:
            rows.append((p[t] - y[t]) ** 2)
        elif prob_form:
            pc = torch.clamp(p[t], EPS, 1.0 - EPS)
            rows.append(-(y[t] * torch.log(pc + EPS) + (1.0 - y[t]) * torch.log(1.0 - pc + EPS)))
        else:
            rows.append(torch.relu(z[t]) - z[t] * y[t] + torch.log1p(torch.exp(-torch.abs(z[t]))))
    return torch.stack(rows)


def weighted_sum(terms, w, scale, reduction):
    """Σ_t a_t (Σ_b w l) / denom_t on torch float64 [T, B]; zero weights select their entries out."""
    T, B = terms.shape
    w = torch.as_tensor(w, dtype=torch.float64)
    sel = torch.where(w > 0, w * terms, torch.zeros_like(terms))
    num = sel.sum(1)
    den = torch.full((T,), float(B), dtype=torch.float64) if reduction == 'batch' else w.sum(1)
    a = torch.ones(T, dtype=torch.float64) if scale is None else torch.as_tensor(scale, dtype=torch.float64)
    per = torch.where(den > 0, a * num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))
    return per.sum(), den.numpy()


def kernel_ref(z, p, y, w, mse_mask, scale, reduction, prob_form, gscale):
    """(loss, gradient [T, B], denom [T]) of the kernel-level call on f32 arrays.  The gradient is taken with respect
    to the logits (p = sigmoid(z) inside the MSE tasks, as the model computes it) or, ``prob_form``, to the
    probabilities.  ``w``: [T, B] raw weights (clamped here); zero-weight entries may hold anything."""
    T, B = y.shape
    wc = np.broadcast_to(clamp_weights(w), (T, B)).copy()
    live = wc > 0
    mse = [(mse_mask >> t) & 1 for t in range(T)]
    yt = torch.from_numpy(np.where(live, y, 0.0).astype(np.float64))
    if prob_form:
        leaf = torch.from_numpy(np.where(live, p, 0.5).astype(np.float64)).requires_grad_(True)
        pt, zt = leaf, None
    else:
        leaf = torch.from_numpy(np.where(live, z, 0.0).astype(np.float64)).requires_grad_(True)
        zt = leaf
        # the loss value uses the f32 probabilities the kernel is given; the gradient flows through sigmoid(z)
        pt = torch.sigmoid(zt) + (torch.from_numpy(np.where(live, p, 0.5).astype(np.float64)) - torch.sigmoid(zt)).detach()
    loss, den = weighted_sum(_terms(yt, pt, zt, mse, prob_form), wc, scale, reduction)
    (loss * gscale).backward()
    g = leaf.grad.numpy().copy()         # (probability form: torch.clamp's gradient is 0 outside [eps, 1 - eps], as Keras's)
    return loss.item(), g, den, wc


def model_loss_and_grads(P, cfg, ns, seq, labels, weights, scale=None, reduction='batch'):
    """The float64 oracle's forward, the weighted loss on its logits / probabilities ([B, 1] labels: the logits form),
    and every parameter's gradient.  ``weights`` [T, B]; labels at zero-weight entries may be NaN."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in R.to_torch(P).items()}
    out = R.forward(leaves, cfg, R.to_torch(ns), R.to_torch(seq), training=False)
    T = len(cfg.tasks)
    wc = clamp_weights(weights)
    y = np.stack([np.asarray(labels[t], dtype=np.float64).reshape(-1) for t in cfg.tasks])
    yt = torch.from_numpy(np.where(wc > 0, y, 0.0))
    z = torch.stack([out['logits'][t].reshape(-1) for t in cfg.tasks])
    p = torch.stack([out['probs'][t].reshape(-1) for t in cfg.tasks])
    mse = [t not in ('ctr', 'cvr') for t in cfg.tasks]
    loss, _ = weighted_sum(_terms(yt, p, z, mse, False), wc, scale, reduction)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.item(), grads, p.detach()


def ref_state_weighted(y, p, w, bnd):
    """counts [T, 2, nb+1] int64 and sums [T, 4] float64 in units of 2^-24 of [T, B] f32 labels / probabilities under
    weights [T, B] (or [B]); zero-unit samples are skipped whatever they hold."""
    y, p = np.asarray(y, dtype=np.float32), np.asarray(p, dtype=np.float32)
    T, nb = y.shape[0], len(bnd)
    u = np.broadcast_to(units(w), y.shape)
    counts = np.zeros((T, 2, nb + 1), dtype=np.int64)
    sums = np.zeros((T, 4), dtype=np.float64)
    for t in range(T):
        k = u[t] > 0
        p64, y64, uu = p[t][k].astype(np.float64), y[t][k].astype(np.float64), u[t][k]
        b = (p64[None, :] > bnd[:, None]).sum(0)
        np.add.at(counts[t], ((y[t][k] > 0.5).astype(np.int64), b), uu)
        d = p64 - y64
        pc = np.clip(p64, EPS, 1.0 - EPS)
        bce = -(y64 * np.log(pc + EPS) + (1.0 - y64) * np.log(1.0 - pc + EPS))
        uf = uu.astype(np.float64)
        sums[t] = [float(uu.sum()), np.sum(uf * (d * d)), np.sum(uf * np.abs(d)), np.sum(uf * bce)]
    return counts, sums


def _div(a, b):
    return float(a) / float(b) if b > 0 else 0.0


def weighted_metrics(y, p, w, thresholds, binary=True):
    """One task's Keras metrics under sample weights, straight from the samples (weights in metric units)."""
    y, p = np.asarray(y, dtype=np.float32), np.asarray(p, dtype=np.float32)
    u = units(w).astype(np.float64)
    k = u > 0
    y64, p64, u = y[k].astype(np.float64), p[k].astype(np.float64), u[k]
    d = p64 - y64
    if not binary:
        return {'mse': _div(np.sum(u * d * d), u.sum()), 'mae': _div(np.sum(u * np.abs(d)), u.sum())}
    pos, pred = y64 > 0.5, p64 > 0.5
    tp, fp = u[pred & pos].sum(), u[pred & ~pos].sum()
    fn, tn = u[~pred & pos].sum(), u[~pred & ~pos].sum()
    prec, rec = _div(tp, tp + fp), _div(tp, tp + fn)
    tps = np.array([u[(p64 > th) & pos].sum() for th in thresholds])
    fps = np.array([u[(p64 > th) & ~pos].sum() for th in thresholds])
    P, N = u[pos].sum(), u[~pos].sum()
    tpr = np.array([_div(a, P) for a in tps])
    fpr = np.array([_div(a, N) for a in fps])
    pc = np.clip(p64, EPS, 1.0 - EPS)
    bce = -(y64 * np.log(pc + EPS) + (1.0 - y64) * np.log(1.0 - pc + EPS))
    return {'auc': float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0)),
            'accuracy': _div(tp + tn, u.sum()), 'precision': prec, 'recall': rec,
            'f1': _div(2.0 * prec * rec, prec + rec), 'logloss': _div(np.sum(u * bce), u.sum())}
