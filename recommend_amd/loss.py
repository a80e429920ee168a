"""The training losses of OneTransModel's heads (reference train.py:78-93, 124-128): three autograd ops over the
loss kernels and ``keras_bce_loss``, which picks among them."""

from __future__ import annotations

import torch

from . import _lib
from . import kernels as K


class _TaskLoss(torch.autograd.Function):
    """Σ_task loss (train.py:78-93, 124-128) of the model's heads as the reference's Keras 2.12 computes it:
    the sigmoid heads' cached logits give tf.nn.sigmoid_cross_entropy_with_logits for 'ctr' / 'cvr' (no
    clipping), MeanSquaredError on the probabilities for any other task; the gradient goes to the logits."""

    @staticmethod
    def forward(ctx, probs, logits, labels, mse_mask):
        T, B = probs.shape
        loss = torch.empty(1, device=probs.device)
        K.task_loss_logits_fwd(logits, probs, labels, T, B, loss, device=probs.device, mse_mask=mse_mask)
        ctx.save_for_backward(probs, labels)
        ctx.mse_mask = mse_mask
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        probs, labels = ctx.saved_tensors
        T, B = probs.shape
        dlogits = torch.empty_like(probs)
        gl = gl.reshape(1).contiguous().float()
        K.task_loss_logits_bwd(probs, labels, gl, T, B, dlogits, mse_mask=ctx.mse_mask)
        return None, dlogits, None, None


class _BCE(torch.autograd.Function):
    """Σ_task loss (train.py:78-93, 124-128) on probs [T, B]: tf.keras BinaryCrossentropy for 'ctr' /
    'cvr', MeanSquaredError for any other task (bit t of ``mse_mask``)."""

    @staticmethod
    def forward(ctx, probs, labels, mse_mask):
        T, B = probs.shape
        loss = torch.empty(1, device=probs.device)
        K.bce_fwd(probs, labels, T, B, loss, device=probs.device, mse_mask=mse_mask)
        ctx.save_for_backward(probs, labels)
        ctx.mse_mask = mse_mask
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        probs, labels = ctx.saved_tensors
        T, B = probs.shape
        dprobs = torch.empty_like(probs)
        gl = gl.reshape(1).contiguous().float()
        K.bce_bwd(probs, labels, gl, T, B, dprobs, mse_mask=ctx.mse_mask)
        return dprobs, None, None


class _WeightedTaskLoss(torch.autograd.Function):
    """Σ_t a_t (Σ_b w l) / denom_t: the per-element terms of ``_TaskLoss`` (``logits`` given: the
    gradient goes to the logits) or of ``_BCE`` (``logits`` None: to the probabilities) under per-(task, sample)
    weights.  The forward leaves the denominators on the device for the backward: no host sync."""

    @staticmethod
    def forward(ctx, probs, logits, labels, weights, wstride, task_scale, mse_mask, reduction):
        T, B = probs.shape
        loss = torch.empty(1, device=probs.device)
        denom = torch.empty(T, device=probs.device)
        K.task_loss_weighted_fwd(logits, probs, labels, weights, wstride, task_scale, T, B, loss, denom,
                                 device=probs.device, mse_mask=mse_mask, reduction=reduction)
        ctx.save_for_backward(probs, labels, weights, denom, task_scale)
        ctx.args = (wstride, mse_mask, logits is None)
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        probs, labels, weights, denom, task_scale = ctx.saved_tensors
        wstride, mse_mask, prob_form = ctx.args
        T, B = probs.shape
        dout = torch.empty_like(probs)
        gl = gl.reshape(1).contiguous().float()
        K.task_loss_weighted_bwd(probs, labels, weights, wstride, task_scale, denom, gl, T, B, dout,
                                 mse_mask=mse_mask, prob_form=prob_form)
        return (dout, None) + (None,) * 6 if prob_form else (None, dout) + (None,) * 6


BINARY_TASKS = ('ctr', 'cvr')      # train.py:83: BCE for these, MSE for every other task


def task_mse_mask(tasks) -> int:
    """Bit t set when task t trains with MeanSquaredError (train.py:88-91)."""
    if len(tasks) > 32:
        raise ValueError('at most 32 tasks')
    return sum(1 << i for i, t in enumerate(tasks) if t not in BINARY_TASKS)


def keras_bce_loss(labels: torch.Tensor, probs: torch.Tensor, tasks=None, label_rank: int = 2, weights=None,
                   task_scale=None, reduction: str = 'batch') -> torch.Tensor:
    """Sum over tasks of the reference's per-task loss; labels/probs [T, B] device tensors.  ``tasks``
    (names, in row order) selects MSE for tasks other than 'ctr'/'cvr'; None = BCE for every row.
    Probabilities from ``OneTransModel.forward_probs`` carry their heads' logits (``_ot_logits``, as Keras's
    sigmoid output carries ``_keras_logits``) and the BCE is taken from those when the caller's labels were
    [B, 1] (``label_rank`` 2: create_sample_batch, data_loader.py:327).  Keras 2.12 squeezes the [B, 1]
    prediction to [B] for [B] labels (get_tf_dataset's batched scalars, data_loader.py:215-218), which drops
    the cached logits: ``label_rank`` 1 and probabilities without logits use the clipped probability form.

    ``weights`` (float32 device tensor: [T, B], or [B] / [1, B] shared by the tasks; values in [0, 65536], a zero
    removes the entry whatever its label holds), ``task_scale`` (T coefficients a_t: a sequence or a device tensor)
    and ``reduction`` ('batch': Σ_t a_t Σ_b w l / B, Keras's SUM_OVER_BATCH_SIZE with ``sample_weight``; 'weights':
    ... / Σ_b w) select the weighted loss.  With ``weights`` None the call is the un-weighted one;
    ``task_scale`` / ``reduction`` then need weights (pass ones)."""
    mask = task_mse_mask(tasks) if tasks is not None else 0
    z = getattr(probs, '_ot_logits', None) if label_rank >= 2 else None
    if weights is None and (task_scale is not None or reduction != 'batch'):
        raise ValueError('keras_bce_loss: task_scale / reduction apply to the weighted loss; pass weights')
    if weights is not None:
        T, B = probs.shape
        if reduction not in _lib.LOSS_REDUCTIONS:
            raise ValueError(f"unknown reduction {reduction!r}: expected 'batch' or 'weights'")
        if weights.dtype != torch.float32 or weights.device != probs.device:
            raise ValueError('keras_bce_loss: weights must be a float32 tensor on the device of probs')
        if weights.dim() == 2 and tuple(weights.shape) == (T, B) and T > 1:
            # (an expanded [1, B] row stays one row: weight stride 0)
            weights, wstride = (weights[0].contiguous(), 0) if weights.stride(0) == 0 else (weights.contiguous(), B)
        elif weights.numel() == B:
            weights, wstride = weights.reshape(-1).contiguous(), 0
        else:
            raise ValueError(f'keras_bce_loss: weights of shape {tuple(weights.shape)}; expected [{T}, {B}] or [{B}]')
        if task_scale is not None and not isinstance(task_scale, torch.Tensor):
            task_scale = torch.tensor([float(a) for a in task_scale], dtype=torch.float32, device=probs.device)
        if task_scale is not None and (task_scale.numel() != T or task_scale.dtype != torch.float32):
            raise ValueError(f'keras_bce_loss: task_scale must hold {T} float32 coefficients')
        return _WeightedTaskLoss.apply(probs, z, labels, weights, wstride, task_scale, mask, reduction)
    if z is not None:
        return _TaskLoss.apply(probs, z, labels, mask)
    return _BCE.apply(probs, labels, mask)
