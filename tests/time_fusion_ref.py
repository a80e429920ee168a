"""Yardstick of timestamp-aware sequence fusion (``OneTransConfig.seq_fusion = 'time'``), numpy / torch on the CPU.

* ``merge_ranks``: the order itself — per sample the stable sort of all events by (time, index of the sequence,
  position in the sequence), as a rank per event in concatenation order.
* ``tokenizer_time``: the oracle's tokenizer (oracle/onetrans_ref.py) with the S part replaced by the per-sequence
  projections, no [SEP], permuted per sample into that order.  Tests install it over ``oracle.onetrans_ref.tokenizer``
  with pytest's monkeypatch; the oracle's forward / loss_and_grads / train_step then run time-fused in float64.
"""

import numpy as np
import torch

from oracle import onetrans_ref as R

_sep_tokenizer = R.tokenizer            # the oracle's own, taken before any test patches the module


def merge_ranks(times_list):
    """``times_list``: one integer [B, L_i] array per present sequence, in configuration order.  Returns int64
    [B, sum L_i]: entry (b, start_i + j) is the place of event j of sequence i in sample b's time order."""
    times_list = [np.asarray(t).astype(np.int64) for t in times_list]
    B = times_list[0].shape[0]
    t = np.concatenate(times_list, axis=1)
    seq = np.concatenate([np.full(x.shape[1], i) for i, x in enumerate(times_list)])
    pos = np.concatenate([np.arange(x.shape[1]) for x in times_list])
    ranks = np.empty(t.shape, dtype=np.int64)
    for b in range(B):
        order = np.lexsort((pos, seq, t[b]))            # the last key is the primary one
        ranks[b, order] = np.arange(t.shape[1])
    return ranks


def tokenizer_time(P, cfg, ns, seq):
    """[S tokens in time order ; NS tokens] -> [B, L_S + L_NS, d], L_S = sum L_i."""
    names = [n for n in cfg.feature_config['sequence_features'] if n in seq]
    B = (next(iter(ns.values())) if ns else seq[names[0]]).shape[0]
    d = cfg.hidden_dim
    dtype = P['tok.ns.kernel'].dtype
    ns_tok = _sep_tokenizer(P, cfg, ns, {}) if ns else torch.zeros(B, cfg.num_ns_tokens, d, dtype=dtype)
    if not names:
        return ns_tok
    parts, times = [], []
    for name in names:
        i = cfg.feature_config['sequence_features'].index(name)
        v = seq[name]
        if cfg.seq_item_vocab and not torch.is_floating_point(v):
            v = P['emb.seq_item'][v.long()]
        parts.append(v.to(dtype) @ P['tok.seq.kernel'][i] + P['tok.seq.bias'][i])
        times.append(np.asarray(seq[name + cfg.seq_time_suffix]))
    cat = torch.cat(parts, dim=1)                                    # concatenation order
    order = np.argsort(merge_ranks(times), axis=1)                   # order[b, r] = the event at place r
    s_tok = cat[torch.arange(B)[:, None], torch.from_numpy(order)]
    return torch.cat([s_tok, ns_tok], dim=1)
