"""Yardstick of the key-padding mask (``OneTransConfig.seq_padding_mask``), float64 numpy / torch on the CPU.

Behaviour sequences arrive left-padded to their cap; ``lens[name + cfg.seq_len_suffix]`` [B] counts each sample's real
events, which are the last ``len`` positions.  Token validity over layer 0's tokens: [SEP] and NS tokens are valid,
event j of a sequence of cap L is valid iff j >= L - len.  Query at position i sees key j iff j <= i and (valid[j] or
j == i).

* ``valid0_np``: the validity array for both fusion modes ('time': an event sits at its rank in the time order,
  tests/time_fusion_ref.merge_ranks).
* ``forward`` / ``loss_and_grads``: the oracle's model (oracle/onetrans_ref.py: its tokenizer, norms, grouped products,
  dropout and heads, imported; its tail-keep block restated here with the visibility rule above; under 'time' the
  tokenizer of tests/time_fusion_ref.py), with autograd for the gradients.
* ``truncate``: sample b's un-padded inputs — what the untouched oracle is run on to pin the semantics: with
  ``dedicated_positions='tail'`` and no pruning the S tokens share one weight group and carry no positional term, so
  the masked model on a padded sample equals the un-masked model on that sample's real events.
"""

import math

import numpy as np
import torch

from oracle import onetrans_ref as R
from time_fusion_ref import merge_ranks, tokenizer_time


def seq_layout(cfg, seq):
    """(present sequence names, caps, first token positions under 'sep', L_S) for the arrays in ``seq``."""
    names_cfg = cfg.feature_config['sequence_features']
    time = getattr(cfg, 'seq_fusion', 'sep') == 'time'
    names, caps, offs, pos = [], [], [], 0
    for i, n in enumerate(names_cfg):
        if n not in seq:
            continue
        L = int(np.asarray(seq[n]).shape[1])
        names.append(n); caps.append(L); offs.append(pos)
        pos += L
        if i < len(names_cfg) - 1 and not time:
            pos += 1                                         # the [SEP] after every sequence but the last configured
    return names, caps, offs, pos


def valid0_np(cfg, seq, lens) -> np.ndarray:
    """uint8 [B, L0]: validity of layer 0's tokens (lengths clamped to [0, cap])."""
    names, caps, offs, L_S = seq_layout(cfg, seq)
    B = np.asarray(seq[names[0]]).shape[0] if names else np.asarray(next(iter(lens.values()))).shape[0]
    valid = np.ones((B, L_S + cfg.num_ns_tokens), dtype=np.uint8)
    if not names:
        return valid
    sfx = cfg.seq_len_suffix
    ev = [np.arange(L)[None, :] >= L - np.clip(np.asarray(lens[n + sfx]).reshape(B, 1), 0, L)
          for n, L in zip(names, caps)]
    if getattr(cfg, 'seq_fusion', 'sep') == 'time':
        ranks = merge_ranks([np.asarray(seq[n + cfg.seq_time_suffix]) for n in names])   # [B, L_S], concat order
        cat = np.concatenate(ev, axis=1)
        np.put_along_axis(valid, ranks, cat.astype(np.uint8), axis=1)
    else:
        for e, L, off in zip(ev, caps, offs):
            valid[:, off:off + L] = e
    return valid


def block_masked(P, cfg, l, x, keep, training, seed, valid):
    """oracle/onetrans_ref.block_vectorized (tail keep) with the key-padding mask ``valid`` [B, I] (bool)."""
    B, I, d = x.shape
    H = cfg.num_heads
    hd = d // H
    rate = cfg.dropout_rate
    groups = torch.tensor([cfg.group_of_position(i, I) for i in range(I)])
    tail = np.arange(I - keep, I)
    gt = groups[I - keep:]
    xn = R.rmsnorm(x, P[f'blk.{l}.norm1'])
    W = P[f'blk.{l}.wqkv']
    kv = R._grouped_mm(xn, W[:, :, d:], groups)
    q = R._grouped_mm(xn[:, I - keep:], W[:, :, :d], gt)
    k, v = kv[..., :d], kv[..., d:]
    qh = q.reshape(B, keep, H, hd); kh = k.reshape(B, I, H, hd); vh = v.reshape(B, I, H, hd)
    s = torch.einsum('bqhd,bkhd->bhqk', qh, kh) / math.sqrt(hd)
    qpos = torch.arange(I - keep, I)[:, None]
    kpos = torch.arange(I)[None, :]
    vis = (kpos <= qpos)[None] & (valid[:, None, :] | (kpos == qpos)[None])           # [B, keep, I]
    s = torch.where(vis[:, None], s, torch.tensor(-math.inf, dtype=s.dtype))
    o = torch.einsum('bhqk,bkhd->bqhd', torch.softmax(s, -1), vh).reshape(B, keep, d)
    a = o @ P[f'blk.{l}.wo']
    xt = x[:, I - keep:] + R.apply_dropout(a, training, rate, seed, 2 * l, I, tail)
    xn2 = R.rmsnorm(xt, P[f'blk.{l}.norm2'])
    h = R.gelu(R._grouped_mm(xn2, P[f'blk.{l}.w1'], gt, P[f'blk.{l}.b1']))
    f = R._grouped_mm(h, P[f'blk.{l}.w2'], gt, P[f'blk.{l}.b2'])
    return xt + R.apply_dropout(f, training, rate, seed, 2 * l + 1, I, tail)


def forward(P, cfg, ns, seq, lens, training=False, seed=0):
    """oracle/onetrans_ref.forward with the mask; ``seq`` holds the padded arrays (and the times under 'time') as
    torch tensors, ``lens`` the numpy / torch lengths.  Tail keeps only."""
    assert getattr(cfg, 'pyramid_select', 'tail') == 'tail'
    time = getattr(cfg, 'seq_fusion', 'sep') == 'time'
    x = (tokenizer_time if time else R.tokenizer)(P, cfg, ns, seq)
    np_seq = {k: np.asarray(v) for k, v in seq.items()}
    valid0 = torch.from_numpy(valid0_np(cfg, np_seq, {k: np.asarray(v) for k, v in lens.items()}).astype(bool))
    L0 = x.shape[1]
    assert valid0.shape[1] == L0
    sched = cfg.pyramid_schedule(L0)
    nl = len(sched)
    for l, s in enumerate(sched):
        I, keep = s['in_len'], s['keep']
        assert x.shape[1] == I
        x = block_masked(P, cfg, l, x, keep if l < nl - 1 else 1, training, seed, valid0[:, L0 - I:])
    out = R.rmsnorm(x, P['out_norm'])
    last = out[:, -1, :]
    probs, logits = {}, {}
    for ti, t in enumerate(cfg.tasks):
        h = R.gelu(last @ P['head.w1'][ti] + P['head.b1'][ti])
        z = (h @ P['head.w2'][ti] + P['head.b2'][ti]).reshape(-1, 1)
        logits[t] = z
        probs[t] = torch.sigmoid(z)
    return {'probs': probs, 'logits': logits}


def loss_and_grads(P, cfg, ns, seq, lens, labels, training=True, seed=0):
    """oracle/onetrans_ref.loss_and_grads over the masked forward ([B, 1] labels: the logits form of the BCE)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    out = forward(leaves, cfg, ns, seq, lens, training=training, seed=seed)
    loss = 0.0
    for t in cfg.tasks:
        y = labels[t].to(out['probs'][t].dtype)
        z = out['logits'][t] if y.dim() >= 2 else None
        loss = loss + R.task_loss(t, y.reshape(-1), out['probs'][t].reshape(-1), None if z is None else z.reshape(-1))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.detach(), grads, out


def truncate(cfg, ns, seq, lens, b):
    """Sample b alone with its un-padded sequences (numpy): ({name: [1, ...]}, {name: [1, len_b, ...]})."""
    names, caps, _, _ = seq_layout(cfg, seq)
    ns1 = {k: np.asarray(v)[b:b + 1] for k, v in ns.items()}
    seq1 = {}
    for n, L in zip(names, caps):
        ln = int(np.clip(np.asarray(lens[n + cfg.seq_len_suffix]).reshape(-1)[b], 0, L))
        seq1[n] = np.asarray(seq[n])[b:b + 1, L - ln:]
    return ns1, seq1
