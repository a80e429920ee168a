"""OneTransModel on MI355X: the reference ``OneTransModel`` (model.py:305-416) as a torch
``nn.Module`` whose every arithmetic step runs in libonetrans_hip.so.

Drop-in surface: ``OneTransModel(config)``;
``forward(non_seq_features, seq_features=None, training=None, use_kv_cache=False) ->
{task: probs [B,1]}``, also accepting the callers' tuple form ``model((non_seq, seq),
training=...)`` (train.py:118, evaluate.py:87 — defect D4); ``reset_kv_cache()``;
``get_model_info()``; ``trainable_variables``; ``save_weights/load_weights``;
``create_onetrans_model(model_type)``.

Autograd: four ``torch.autograd.Function``s (tokenizer and output-norm+heads here, the block in block.py,
the losses in loss.py).  Their backward passes write parameter gradients straight into the flat gradient buffer
``model.flat.grad`` (one bank per reference variable group), so the optimizer and the DP
all-reduce each touch one contiguous buffer.  Embedding-table gradients are handed to the
optimizer as (row keys, gradient rows) pairs: sparse updates, never a dense table gradient.
"""

from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from ._lib import OT_EPI_ACCUMULATE, OT_EPI_BIAS, OT_GEMM_NT, NS_FIELD_BYTES
from .block import RMS_EPS, PairBounds, _Block, layer_seed
from .config import (OneTransConfig, check_bag_features, check_ns_tokenizer, check_padding_mask, check_pyramid_select,
                     check_seq_fusion, check_weighted_loss, get_model_config)
from .layout import TILE, FlatLayout, build_map, head_map, identity_map, layer_maps, round_up
from .loss import BINARY_TASKS, keras_bce_loss  # noqa: F401  (re-exported: callers import them from here)
from .params import init_params, ns_table_offsets

NS_GROUPS_KEY = '__ns_token_groups__'   # save_weights: the groups of a group-wise NS tokenizer (JSON), next to the banks


# =============================================================================== autograd ops
class _Tokenize(torch.autograd.Function):
    """Tokenizer.call (model.py:224-277): [S tokens ; NS tokens] -> x0 [B*L0, d]."""

    @staticmethod
    def forward(ctx, flat, m, plan):
        d = m.config.hidden_dim
        B, L0, L_S = plan['B'], plan['L0'], plan['L_S']
        dev = flat.device
        x0 = torch.empty(B * L0, d, device=dev)
        # ---- NS tokens: gather/concat -> Dense(L_NS*d) straight into token rows L_S.. (model.py:253-254)
        if plan['ns_fields'] > 0:
            nsm = plan['nsmat']
            if plan['ns_desc_n'] > 0:
                K.ns_assemble(plan['ns_desc'], plan['ns_desc_n'], m.tables.get('emb.ns'), B, nsm, m.layout.f_pad)
            if plan['n_bags'] > 0:                              # multi-valued features: pooled rows, same matrix
                K.ns_bag_pool(plan['bag_descs'], plan['n_bags'], B, nsm, m.layout.f_pad, plan['bag_coef'])
            if m.ns_goff is not None:                           # one Dense(F_g -> d) per feature group (paper eq. 6)
                K.ns_group_fwd(nsm, m.layout.f_pad, m.ns_goff, m.config.num_ns_tokens, m.layout.f_pad, m.ns_kmax,
                               m.p('tok.ns.kernel'), m.p('tok.ns.bias'), B, d, (x0, L_S * d), L0 * d)
            else:
                mp = plan['ns_map'].to(dev)
                K.gemm(OT_GEMM_NT, nsm, m.layout.f_pad, m.layout.f_pad, mp['rows'][0], m.pT('tok.ns.kernel'), 0,
                       m.layout.f_pad, m.cfg_Lnsd, mp['tile_group'], plan['ns_map'].ntiles, (x0, L_S * d), L0 * d,
                       mp['rows'][0], bias=m.p('tok.ns.bias'), epi=OT_EPI_BIAS, m_rows=B,
                       bimg=m.bimg('tok.ns.kernel'))
        else:                                                   # model.py:249-251
            x0.view(B, L0, d)[:, L_S:].zero_()
        # ---- S tokens: per-sequence Dense(d) on gathered item rows (model.py:262-265)
        if plan['seq_map'] is not None:
            sm = plan['seq_map'].to(dev)
            A, lda = plan['seq_A'], m.config.seq_feature_dim
            K.gemm(OT_GEMM_NT, A, lda, lda, plan['seq_in'], m.pT('tok.seq.kernel'), lda * d, lda, d, sm['tile_group'],
                   plan['seq_map'].ntiles, x0, d, _seq_out_rows(plan, sm), bias=m.p('tok.seq.bias'), bias_gstride=d,
                   epi=OT_EPI_BIAS, m_rows=plan['seq_M'], bimg=m.bimg('tok.seq.kernel'))
        if plan['n_sep'] > 0:                                   # model.py:270-272
            K.fill_rows(x0, d, plan['sep_rows'], plan['n_sep'], m.p('tok.sep'), d)
        ctx.m, ctx.plan, ctx.gen = m, plan, plan['gen']
        return x0

    @staticmethod
    def backward(ctx, dx0):
        # the autograd engine runs this on its own thread: enter the model's precision there
        with K.precision(ctx.m.matmul):
            return _Tokenize._backward(ctx, dx0)

    @staticmethod
    def _backward(ctx, dx0):
        m, plan = ctx.m, ctx.plan
        if plan['gen'] != ctx.gen:
            raise RuntimeError('OneTransModel: a second forward with the same input shapes ran before this '
                               'backward; run backward before the next forward (inputs are staged in place)')
        dx0 = dx0.contiguous()
        d = m.config.hidden_dim
        B, L0, L_S = plan['B'], plan['L0'], plan['L_S']
        dev = dx0.device
        acc = m.accumulate_grads
        m._pending_sparse = []
        if plan['ns_fields'] > 0:
            mp = plan['ns_map'].to(dev)
            nsm = plan['nsmat']
            grouped = m.ns_goff is not None
            if grouped:
                K.ns_group_bwd_weight(nsm, m.layout.f_pad, (dx0, L_S * d), L0 * d, m.ns_goff, m.config.num_ns_tokens,
                                      m.layout.f_pad, m.ns_kmax, B, d, m.g('tok.ns.kernel'), m.g('tok.ns.bias'),
                                      accumulate=acc, device=dev)
            else:
                K.wgrad(nsm, m.layout.f_pad, mp['rows'][0], (dx0, L_S * d), L0 * d, mp['rows'][0], m.layout.f_pad,
                        m.cfg_Lnsd, mp, plan['ns_map'].chunks.shape[0], 1, m.g('tok.ns.kernel'), 0,
                        m.g('tok.ns.bias'), 0, accumulate=acc, device=dev, m_rows=B, rowmap=plan['ns_map'])
            if plan['n_sparse'] > 0 or plan['n_bags'] > 0:
                dns = torch.empty(B, m.layout.f_pad, device=dev)
                if grouped:
                    K.ns_group_bwd_input((dx0, L_S * d), L0 * d, m.ns_goff, m.config.num_ns_tokens, m.layout.f_pad,
                                         m.ns_kmax, m.p('tok.ns.kernel'), B, d, dns, m.layout.f_pad)
                else:
                    K.gemm(OT_GEMM_NT, (dx0, L_S * d), L0 * d, m.cfg_Lnsd, mp['rows'][0], m.p('tok.ns.kernel'), 0,
                           m.cfg_Lnsd, m.layout.f_pad, mp['tile_group'], plan['ns_map'].ntiles, dns, m.layout.f_pad,
                           mp['rows'][0], m_rows=B)
                e = m.config.ns_embedding_dim
                # one (keys, grads) pair per table: the single-id fields' B entries each, then every slot of the
                # emb.ns bags; the emb.seq_item bags' slots are a second entry of that table (the optimizer joins
                # the entries of one table before it de-duplicates)
                n1 = plan['n_sparse'] * B
                n = n1 + plan['bag_ns_slots']
                if n > 0:
                    keys = torch.empty(n, dtype=torch.int64, device=dev)
                    grads = torch.empty(n, e, device=dev)
                    if n1 > 0:
                        K.ns_grad_pack(plan['ns_desc'], plan['n_sparse'], e, dns, m.layout.f_pad, B, keys, grads)
                    if plan['n_bags_ns'] > 0:
                        K.ns_bag_grad_pack(plan['bag_descs'], plan['n_bags_ns'], B, dns, m.layout.f_pad,
                                           plan['bag_coef'], (keys, n1), (grads, n1 * e))
                    m._pending_sparse.append(('emb.ns', keys, grads))
                nq = plan['n_bags'] - plan['n_bags_ns']
                if nq > 0:
                    Eq = m.config.seq_feature_dim
                    nslots = plan['bag_slots'] - plan['bag_ns_slots']
                    keys = torch.empty(nslots, dtype=torch.int64, device=dev)
                    grads = torch.empty(nslots, Eq, device=dev)
                    K.ns_bag_grad_pack(plan['bag_descs'], nq, B, dns, m.layout.f_pad,
                                       (plan['bag_coef'], plan['bag_ns_slots']), keys, grads, first=plan['n_bags_ns'])
                    m._pending_sparse.append(('emb.seq_item', keys, grads))
        elif not acc:
            m.g('tok.ns.kernel').zero_()
            m.g('tok.ns.bias').zero_()
        E = m.config.seq_feature_dim
        if plan['seq_map'] is not None:
            sm = plan['seq_map'].to(dev)
            xrows = _seq_out_rows(plan, sm)
            K.wgrad(plan['seq_A'], E, plan['seq_in'], dx0, d, xrows, E, d, sm,
                    plan['seq_map'].chunks.shape[0], plan['nseq'], m.g('tok.seq.kernel'), E * d,
                    m.g('tok.seq.bias'), d, accumulate=acc, device=dev, m_rows=plan['seq_M'],
                    rowmap=plan['seq_map'])
            if plan['seq_ids'] is not None:
                M = plan['seq_M']
                demb = torch.empty(M, E, device=dev)
                K.gemm(OT_GEMM_NT, dx0, d, d, xrows, m.p('tok.seq.kernel'), E * d, d, E, sm['tile_group'],
                       plan['seq_map'].ntiles, demb, E, sm['rows'][1], m_rows=plan['seq_M'])
                # a sharded table takes its gradient rows along the lookup's all-to-all route
                keys = plan['seq_route'] if 'emb.seq_item' in m.sharded else plan['seq_ids']
                m._pending_sparse.append(('emb.seq_item', keys, demb))
        elif not acc:
            m.g('tok.seq.kernel').zero_(); m.g('tok.seq.bias').zero_()
        if plan['n_sep'] > 0:
            K.rows_colsum(dx0, d, plan['sep_rows'], plan['n_sep'], d, m.g('tok.sep'), accumulate=acc, device=dev)
        elif not acc:
            m.g('tok.sep').zero_()
        m.join_side_stream()          # last backward of the graph: every block's weight gradients are in
        return None, None, None


def _seq_out_rows(plan, sm):
    """x0 rows of the sequence projection's row map: the static map (``seq_fusion='sep'``), or under 'time' the
    plan's per-call copy that ot_seq_time_rows filled from this call's timestamps (``_plan``)."""
    rows = plan.get('seq_rows_t')
    return rows if rows is not None else sm['rows'][0]


class _Head(torch.autograd.Function):
    """output_norm + task heads on the last token (model.py:384-391): x [B, d] -> probs [T, B]."""

    @staticmethod
    def forward(ctx, flat, x, m):
        cfg = m.config
        d, T = cfg.hidden_dim, len(cfg.tasks)
        dh = d // 2
        B = x.shape[0]
        dev = x.device
        y = torch.empty(B, d, device=dev)
        rstd = torch.empty(B, device=dev)
        K.rmsnorm_fwd(x, d, B, d, rstd, gamma=m.p('out_norm'), y=y, ldy=d, eps=RMS_EPS)
        hm = m.head_rows(B)
        hmd = hm.to(dev)
        pre1 = torch.empty(T * B, dh, device=dev)
        K.gemm(OT_GEMM_NT, y, d, d, hmd['rows'][0], m.pT('head.w1'), d * dh, d, dh, hmd['tile_group'], hm.ntiles,
               pre1, dh, hmd['rows'][1], bias=m.p('head.b1'), bias_gstride=dh, epi=OT_EPI_BIAS, m_rows=hm.nrows)
        logits = torch.empty(T, B, device=dev)
        probs = torch.empty(T, B, device=dev)
        K.head_fwd(pre1, m.p('head.w2'), m.p('head.b2'), T, B, dh, logits, probs)
        ctx.save_for_backward(x, rstd, y, pre1, probs)
        ctx.m = m
        ctx.set_materialize_grads(False)
        m._last_logits = logits
        return probs, logits

    @staticmethod
    def backward(ctx, dprobs, dlogits):
        # the autograd engine runs this on its own thread: enter the model's precision there
        with K.precision(ctx.m.matmul):
            return _Head._backward(ctx, dprobs, dlogits)

    @staticmethod
    def _backward(ctx, dprobs, dlogits):
        x, rstd, y, pre1, probs = ctx.saved_tensors
        m = ctx.m
        cfg = m.config
        d, T = cfg.hidden_dim, len(cfg.tasks)
        dh = d // 2
        B = x.shape[0]
        dev = x.device
        acc = m.accumulate_grads
        dprobs = dprobs.contiguous() if dprobs is not None else None
        dlogits = dlogits.contiguous() if dlogits is not None else None
        if dprobs is None and dlogits is None:
            return None, None, None
        dpre1 = torch.empty(T * B, dh, device=dev)
        K.head_bwd(pre1, m.p('head.w2'), probs, dprobs, T, B, dh, dpre1, m.g('head.w2'), m.g('head.b2'), dh, 1,
                   accumulate=acc, device=dev, dlogits=dlogits)
        hm = m.head_rows(B)
        hmd = hm.to(dev)
        K.wgrad(y, d, hmd['rows'][0], dpre1, dh, hmd['rows'][1], d, dh, hmd, hm.chunks.shape[0], T, m.g('head.w1'),
                d * dh, m.g('head.b1'), dh, accumulate=acc, device=dev, m_rows=hm.nrows)
        im = m.ident_rows(B).to(dev)
        nti = m.ident_rows(B).ntiles
        dy = torch.empty(B, d, device=dev)
        for t in range(T):
            K.gemm(OT_GEMM_NT, (dpre1, t * B * dh), dh, dh, im['rows'][0], (m.p('head.w1'), t * d * dh), 0, dh, d,
                   im['tile_group'], nti, dy, d, im['rows'][0], epi=OT_EPI_ACCUMULATE if t > 0 else 0, m_rows=B)
        dx = torch.empty(B, d, device=dev)
        K.rmsnorm_bwd(dy, d, x, d, m.p('out_norm'), rstd, dx, d, B, d, dgamma=m.g('out_norm'), accumulate=acc,
                      device=dev)
        if m.grad_ready is not None:
            m.grad_ready('head')                # out_norm + heads are final: the DP exchange may start
        return None, dx, None


# =============================================================================== the module
in_model_precision = K.in_model_precision


class OneTransModel(nn.Module):
    """model.py:305-408 on MI355X (see module docstring)."""

    def __init__(self, config: OneTransConfig, device=None, seed: int = 0, init: Optional[Dict] = None):
        super().__init__()
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.OneTransHipError('OneTransModel needs a ROCm GPU (no CPU fallback)')
        self.config = config
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        cfg = config
        if cfg.hidden_dim % cfg.num_heads or (cfg.hidden_dim // cfg.num_heads) not in (16, 32, 64, 128):
            raise ValueError('head_dim must be 16, 32, 64 or 128')
        check_pyramid_select(cfg)
        check_seq_fusion(cfg)
        check_bag_features(cfg)
        check_padding_mask(cfg)
        check_weighted_loss(cfg)
        check_ns_tokenizer(cfg)
        self.padding_mask = bool(getattr(cfg, 'seq_padding_mask', False))
        self.time_fusion = getattr(cfg, 'seq_fusion', 'sep') == 'time'
        # compute_dtype (build knob): 'fp32' (the reference's arithmetic: split or f32 GEMMs, ``matmul`` below),
        # 'bf16', or 'fp8attn' = BASELINE configs[4]'s attention on
        # block-scaled fp8 MFMA (forward QK^T and PV; the backward recomputes in the GEMM mode's precision from
        # the dequantised fp8 operands the training forward leaves in qkv: the straight-through gradient).
        if getattr(cfg, 'compute_dtype', 'fp32') not in ('fp32', 'bf16', 'fp8attn'):
            raise ValueError(f"compute_dtype {cfg.compute_dtype!r}: expected 'fp32', 'bf16' or 'fp8attn'")
        # this model's GEMM / attention arithmetic, passed with every kernel call it makes (the C ABI holds no
        # precision state): 'bf16' for the reduced-precision configs, else the process default at construction
        # ('split', f32-accurate; kernels.set_matmul_mode / ONETRANS_MATMUL)
        if getattr(cfg, 'compute_dtype', 'fp32') in ('bf16', 'fp8attn'):
            self.matmul = 'bf16'
        elif K.matmul_mode() == 'bf16':
            raise ValueError("compute_dtype 'fp32' with the process default matmul 'bf16' (ONETRANS_MATMUL / "
                             "kernels.set_matmul_mode): set config.compute_dtype = 'bf16' for the bf16 arithmetic")
        else:
            self.matmul = K.matmul_mode()
        # activation recompute (config.recompute_blocks): a block keeps only its
        # input for backward and re-runs its forward kernels there (_Block)
        self.recompute = bool(getattr(cfg, 'recompute_blocks', False))
        self.attn_fp8 = getattr(cfg, 'compute_dtype', 'fp32') == 'fp8attn'
        if self.attn_fp8 and cfg.hidden_dim // cfg.num_heads not in (64, 128):
            raise ValueError('fp8 attention needs head_dim 64 or 128')
        # e4m3 terms per attention operand: 2 (default; hi + lo, AUC within north_star's 1e-3 at C5) or 1
        # (plain e4m3); config fp8_terms
        self.fp8_terms = int(getattr(cfg, 'fp8_terms', 2))
        if self.fp8_terms not in (1, 2):
            raise ValueError(f'fp8_terms {self.fp8_terms}: 1 or 2')
        self.f_ns = cfg.ns_input_width()
        # split mode: the FFN2 / FFN1 / Wo dgrad GEMMs on the scaled fp16 pair (pair-form dgrad images, the A rows'
        # maxima from their producers; ONETRANS_PAIR_DGRAD=0: the six-product split)
        self.layout = FlatLayout(cfg, self.f_ns, pair_dgrad=os.environ.get('ONETRANS_PAIR_DGRAD', '1') != '0')
        self.cfg_Lnsd = cfg.num_ns_tokens * cfg.hidden_dim
        # ns_tokenizer='group' (DESIGN.md §7g): the groups' first columns of the NS matrix = first rows of
        # tok.ns.kernel, on the device for the grouped kernels (ot_ns_group_*), and the widest group
        self.ns_goff, self.ns_kmax = None, 0
        if self.layout.ns_groups is not None:
            if cfg.hidden_dim % 4 or cfg.hidden_dim > 512:
                raise ValueError(f"ns_tokenizer='group' needs hidden_dim % 4 == 0 and <= 512, got {cfg.hidden_dim}")
            # (the last group's range runs on over the bank's padding rows f_ns .. f_pad: zero columns of the NS
            # matrix and zero rows of the bank, so nothing changes but that their gradient rows are written, as zeros)
            gp = self.layout.ns_groups['goff'][:-1] + [self.layout.f_pad]
            self.ns_goff = torch.tensor(gp, dtype=torch.int32, device=self.device)
            self.ns_kmax = max(b - a for a, b in zip(gp[:-1], gp[1:]))
        self.flat = nn.Parameter(torch.zeros(self.layout.total, device=self.device))
        self.flat.grad = torch.zeros_like(self.flat)
        self.flatT = torch.zeros(self.layout.total, device=self.device)     # transposed GEMM weight shadow
        self._tdesc = torch.from_numpy(self.layout.transpose_desc.reshape(-1)).to(self.device)
        # pre-split bf16 plane images of the GEMM weight banks (the plane GEMM's B operand, split / bf16 mode);
        # rebuilt with the transposed shadow after every weight update
        self.img = torch.zeros(max(1, self.layout.image_elems), dtype=torch.int16, device=self.device)
        self._img_valid, self._img_mode = False, None
        self._idesc = (torch.from_numpy(self.layout.image_desc.reshape(-1)).to(self.device)
                       if self.layout.image_units else None)
        self.tables: Dict[str, torch.Tensor] = {}
        self.accumulate_grads = False
        # data-parallel hook (OneTransOptimizer): called with a layer index / 'head' when those gradient
        # banks are final in backward, so their all-reduce overlaps the rest of the backward pass
        self.grad_ready = None
        # fuse the RMSNorms into the neighbouring GEMM epilogues.  d == 128 (a tile holds whole rows, every
        # matmul mode): the forward rstd (Wo / FFN2 epilogues) and the norm backward (FFN1 / QKV dgrad
        # epilogues).  d = 256, 512, ...: the forward rstd only, on the split-mode plane GEMM (per-tile row
        # sums + a finishing pass, ``fuse_with``).  The norm2 backward is fused at every d % 128 == 0
        # (``fuse_bwd2``): the FFN2 dgrad epilogue emits per-tile partials of sum_f dU_f (U_f - b1_f)
        # = rstd2 <gamma2 dy, x1>, the one row reduction the FFN1 dgrad epilogue cannot see.  norm1's
        # backward stays row-wise at d > 128 — a row-complete epilogue (each workgroup looping over the
        # row's column tiles, two passes) measured slower than the row-wise kernel at T
        # (tests/test_model_gpu.py::test_fused_norms_match_unfused turns fuse_norms / fuse_bwd2 off for the
        # row-wise reference path)
        self.fuse_norms = config.hidden_dim % TILE == 0
        self.fuse_bwd = self.fuse_norms and config.hidden_dim == TILE
        self.fuse_bwd2 = self.fuse_norms
        # bf16 mode (C5): every activation whose only readers are GEMM / attention operands rounded to bf16 anyway
        # is stored in bf16 by its producer: h = gelu(U), U, dU, dY2, dQKV and the key slices'
        # dQ partials, the normalised QKV / FFN1 inputs for the weight gradients, the fp8 forward's dequantised
        # Q / K / V, the residual stream's copies for the QKV / FFN1 A operands (take_x16 / put_x16)
        self._x16 = None
        # block weight gradients run on a second stream, overlapping the dgrad chain
        self.overlap_wgrad = True            # bench.py --no-overlap turns it off for standalone kernel traces
        # split mode: weight gradients on the scaled fp16 pair (ot_mixed_gemm_wgrad_ex) wherever the operands'
        # producers report a magnitude bound (PairBounds, one per forward that a backward can follow;
        # ONETRANS_PAIR_WGRAD=0: the exact six-product split everywhere)
        self.pair_wgrad = os.environ.get('ONETRANS_PAIR_WGRAD', '1') != '0'
        self._side = None
        self._side_used = False
        self._side_keep: List[torch.Tensor] = []
        self._side_fifo: List = []
        self.kv_cache = None                      # model.py:333 (reference attribute; never populated)
        self._pending_sparse: List = []
        self._plans: Dict = {}
        self._maps: Dict = {}
        self._aux_maps: Dict = {}
        self._step = 0
        self.dropout_seed = 0x5EED0000 ^ seed
        self.sample_offset: Optional[int] = None      # global index of the local batch's first sample
        # producer of device-resident input ids (row-sharded lookups route them on a side stream): None =
        # the current stream, a HIP event, or True = already complete (resident batches, bench.py)
        self.inputs_ready = None
        # row-sharded tables (data-parallel runs): 'emb.seq_item' lives partitioned over the ranks
        self.sharded: Dict[str, 'ShardedTable'] = {}
        self._pending_route = None                    # route_ahead(): the next lookup's routed ids
        self.last_table_ids: Dict[str, torch.Tensor] = {}   # the forward's ids per replicated table (DP mask)
        shard_seq = self._shard_seq_table()
        params = init if init is not None else init_params(cfg, self.f_ns, seed=seed, with_tables=False)
        if shard_seq:
            from .sharded import ShardedTable
            import torch.distributed as dist
            full = params.get('emb.seq_item') if init is not None else None
            params = {k: v for k, v in params.items() if k != 'emb.seq_item'}
            dist_on = dist.is_available() and dist.is_initialized()
            st = ShardedTable('emb.seq_item', cfg.seq_item_vocab, cfg.seq_feature_dim,
                              dist.get_world_size() if dist_on else 1, dist.get_rank() if dist_on else 0,
                              self.device, seed=seed + 2, full_init=full, route_stream=self.comm_stream())
            self.sharded['emb.seq_item'] = st
            self.tables['emb.seq_item'] = st.table
        self.load_param_dict(params)
        if init is None or not any(k.startswith('emb.') for k in init):
            self._init_tables_device(seed + 1)

    # ---------------------------------------------------------------- parameter access
    def p(self, name):
        return self.layout.view(self.flat.data, name)

    def g(self, name):
        return self.layout.view(self.flat.grad, name)

    def pT(self, name):
        return self.layout.tview(self.flatT, name)

    @in_model_precision
    def refresh_shadow(self) -> None:
        """Re-derive the transposed weight banks after any change of the weights (init, load, optimizer)."""
        K.transpose_banks(self.flat.data, self.flatT, self._tdesc, self.layout.transpose_desc.shape[0],
                          self.layout.transpose_tiles)
        # the plane images feed the plane GEMMs of the split mode (three planes) and the bf16 mode (plane
        # 0 rounded to nearest); built for the current matmul mode, rebuilt lazily if it changes (bimg)
        self._img_valid = False
        if self._idesc is not None and K.matmul_mode() in ('split', 'bf16'):
            self._build_images()

    def _build_images(self) -> None:
        K.split_images(self.flat.data, self._idesc, self.layout.image_desc.shape[0], self.layout.image_units,
                       self.img)
        self._img_valid = True
        self._img_mode = K.matmul_mode()

    def fuse_with(self, *images) -> bool:
        """Run the forward row-norm epilogue (OT_EPI_ROW_RSTD) on GEMMs whose B operands are ``images``
        ((bank, orient) pairs)?  d == 128: always (when fusing is on); d > 128: only on the plane GEMM
        (split mode, every image present)."""
        if not self.fuse_norms:
            return False
        if self.config.hidden_dim == TILE:
            return True
        return all(self.bimg(n, o) is not None for (n, o) in images)

    @property
    def pair_dgrad(self) -> bool:
        """ONETRANS_PAIR_DGRAD as the layout's images were built with it (read-only: the images do not change)."""
        return self.layout.pair_dgrad

    def gemm_pair(self, name: str, orient: str) -> bool:
        """Is ``name``'s ``orient`` image one of the scaled-fp16-pair forms that need the A rows' maxima (a_row_bounds:
        the dgrad images and the Wo forward image under ONETRANS_PAIR_DGRAD, split mode)?"""
        return (K.matmul_mode() == 'split' and (name, orient) in self.layout.pair_images
                and self.bimg(name, orient) is not None and not (orient == 'fwd' and not name.endswith('.wo')))

    def dgrad_pair(self, name: str) -> bool:
        """Is ``name``'s dgrad image in the scaled-fp16-pair form, so its dgrad GEMM must get its A rows' maxima?"""
        return self.gemm_pair(name, 'dgrad')

    def x16_on(self, d: int) -> bool:
        """Store bf16 copies of the residual stream for the next GEMM's A (bf16 mode, plane GEMMs)?"""
        return d % TILE == 0 and K.matmul_mode() == 'bf16'

    def put_x16(self, layer: int, x: torch.Tensor, x16: Optional[torch.Tensor]) -> None:
        """Block ``layer - 1``'s output x and its bf16 copy, for block ``layer``."""
        self._x16 = (layer, x, x.data_ptr(), x.numel(), x16) if x16 is not None else None

    def take_x16(self, layer: int, x: torch.Tensor) -> Optional[torch.Tensor]:
        """The bf16 copy of x that block ``layer - 1``'s FFN2 epilogue stored, if x is that output."""
        c, self._x16 = self._x16, None
        if (c is None or c[0] != layer or not self.x16_on(x.shape[-1]) or c[2] != x.data_ptr()
                or c[3] != x.numel()):
            return None
        return c[4]

    def bimg(self, name: str, orient: str = 'fwd', tn0: int = 0):
        """(image, column tiles per group, first tile) of a weight bank's pre-split B image for the plane
        GEMM: orient 'fwd' = W^T (RMSNorm gamma folded in for wqkv / w1), 'dgrad' = W; None when the
        bank has no image (partial column tiles) or the plane GEMM is off."""
        e = self.layout.images.get((name, orient))
        if e is None:
            return None
        mode = K.matmul_mode()
        if mode not in ('split', 'bf16'):
            return None
        if not self._img_valid or self._img_mode != mode:
            self._build_images()
        off, G, N, K_ = e
        return ((self.img, off), N // TILE, tn0)

    def load_param_dict(self, params: Dict[str, np.ndarray]) -> None:
        """Load host arrays (params.init_params layout; tok.ns.kernel may be unpadded)."""
        with torch.no_grad():
            for name, arr in params.items():
                if name in self.sharded:
                    # row-sharded: keep only this rank's rows (id % world == rank) in the shard the
                    # lookups and updates use; self.tables[name] stays that shard
                    st = self.sharded[name]
                    arr = np.asarray(arr)
                    if arr.shape != (st.num_rows, st.E):
                        raise ValueError(f'{name}: loaded shape {arr.shape} != ({st.num_rows}, {st.E})')
                    st.table[:st.local_rows].copy_(torch.as_tensor(arr[st.rank::st.world], dtype=torch.float32))
                    self.tables[name] = st.table
                    continue
                if name.startswith('emb.'):
                    # the gather kernels trust the configured row counts: a table of another shape (a checkpoint
                    # of another config) is refused here instead of being read out of range
                    want = self._table_shape(name)
                    if want is not None and tuple(np.shape(arr)) != want:
                        raise ValueError(f'{name}: loaded shape {tuple(np.shape(arr))} != {want} of this config')
                    self.tables[name] = torch.as_tensor(np.asarray(arr), dtype=torch.float32).to(self.device).contiguous()
                    continue
                dst = self.p(name)
                src = torch.as_tensor(np.asarray(arr), dtype=torch.float32)
                if name in ('tok.ns.kernel', 'tok.ns.bias'):
                    self._check_ns_bank(name, tuple(src.shape))
                if name == 'tok.ns.kernel' and src.shape[0] != dst.shape[0]:
                    dst.zero_()
                    dst[:src.shape[0]].copy_(src)
                else:
                    dst.copy_(src.reshape(dst.shape))
        self.refresh_shadow()

    def _check_ns_bank(self, name: str, shape) -> None:
        """A loaded NS tokenizer bank must have this model's tokenizer mode: the auto-split bank is
        [F_ns, L_NS*d] / [L_NS*d], the grouped one [F_ns, d] / [L_NS, d]."""
        cfg = self.config
        L, d = cfg.num_ns_tokens, cfg.hidden_dim
        if self.layout.ns_groups is not None:
            want = ('%d or %d' % (self.f_ns, self.layout.f_pad), d) if name == 'tok.ns.kernel' else (L, d)
            ok = (len(shape) == 2 and shape[0] in (self.f_ns, self.layout.f_pad) and shape[1] == d
                  if name == 'tok.ns.kernel' else shape == want)
        else:
            want = ('<= %d' % self.layout.f_pad, L * d) if name == 'tok.ns.kernel' else (L * d,)
            ok = (len(shape) == 2 and shape[0] <= self.layout.f_pad and shape[1] == L * d
                  if name == 'tok.ns.kernel' else int(np.prod(shape)) == L * d)
        if not ok:
            raise ValueError(f"{name}: loaded shape {shape} is not the {want} of ns_tokenizer="
                             f"{getattr(cfg, 'ns_tokenizer', 'auto')!r}: the weights were saved with another NS "
                             'tokenizer mode or other feature groups')

    def _table_shape(self, name: str):
        cfg = self.config
        if name == 'emb.ns':
            return (ns_table_offsets(cfg)['__total__'], cfg.ns_embedding_dim)
        if name == 'emb.seq_item':
            return (cfg.seq_item_vocab, cfg.seq_feature_dim)
        return None

    def param_dict(self) -> Dict[str, np.ndarray]:
        """Host copies of every parameter.  With a row-sharded table this is a COLLECTIVE (the table
        is all-gathered): every rank must call it (``save_weights`` too), not only rank 0."""
        out = {}
        for name in self.layout.shapes:
            v = self.p(name).detach().cpu().numpy().copy()
            if name == 'tok.ns.kernel':
                v = v[:self.f_ns]
            out[name] = v
        for k, t in self.tables.items():
            src = self.sharded[k].full_table() if k in self.sharded else t
            out[k] = src.detach().cpu().numpy().copy()
        return out

    def _shard_seq_table(self) -> bool:
        """Row-shard the sequence-item table?  ``config.table_sharding`` (env ONETRANS_TABLE_SHARDING
        overrides): 'row' always (world 1 outside torch.distributed: one shard, the route as a copy);
        'auto' (default) under torch.distributed with world > 1 when the table exceeds 1 GiB (C4's 100M
        rows; C2's 1M-row table is replicated and exchanged densely)."""
        import torch.distributed as dist
        cfg = self.config
        mode = os.environ.get('ONETRANS_TABLE_SHARDING', getattr(cfg, 'table_sharding', 'auto'))
        if not cfg.seq_item_vocab or mode == 'none':
            return False
        if mode == 'row':
            return True          # (a single process holds the one shard: the route runs, as a copy)
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return False
        return cfg.seq_item_vocab * cfg.seq_feature_dim * 4 > 2 ** 30

    def _init_tables_device(self, seed: int) -> None:
        cfg = self.config
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        total = ns_table_offsets(cfg)['__total__']
        if total:
            t = torch.empty(total, cfg.ns_embedding_dim, device=self.device)
            t.uniform_(-0.05, 0.05, generator=gen)
            self.tables['emb.ns'] = t
        if cfg.seq_item_vocab and 'emb.seq_item' not in self.sharded:
            t = torch.empty(cfg.seq_item_vocab, cfg.seq_feature_dim, device=self.device)
            t.uniform_(-0.05, 0.05, generator=gen)
            self.tables['emb.seq_item'] = t

    @property
    def trainable_variables(self):
        """train.py:131 — the dense parameters (one flat buffer) plus the embedding tables."""
        return [self.flat] + list(self.tables.values())

    # ---------------------------------------------------------------- row maps (cached)
    def maps(self, B, I, Kq, p0=0, I_full=0):
        """Row maps of a block on B samples of I tokens keeping Kq; ``p0`` / ``I_full``: the I rows are the span of
        positions p0.. of a layer of I_full tokens (layout.layer_maps).  A span that is the whole layer shares the
        layer's maps."""
        key = (B, I, Kq) if p0 == 0 and I_full in (0, I) else (B, I, Kq, p0, I_full)
        if key not in self._maps:
            self._maps[key] = layer_maps(self.config, B, I, Kq, p0=p0, I_full=I_full)
        return self._maps[key]

    def fold_ded(self, I: int):
        """(first, end) of the dedicated-group key positions of a layer of I tokens, or None when they are not one
        contiguous run (the folded attention, ot_attn_fold_*, takes them as a range)."""
        key = ('fold', I)
        if key not in self._aux_maps:
            ded = [p for p in range(I) if self.config.group_of_position(p, I) != 0]
            run = (ded[0], ded[-1] + 1) if ded else (0, 0)
            self._aux_maps[key] = run if ded == list(range(*run)) else None
        return self._aux_maps[key]

    def fold_gate(self, I: int, Kq: int, select: bool, masked: bool):
        """Does a block of I tokens keeping Kq take the folded one-query attention?  Its dedicated
        range (``fold_ded``) when it does, else None: the block then runs the K/V projection of every row and the
        attention kernels, exactly as without the switch (ONETRANS_LAST_FOLD / K.last_fold)."""
        cfg = self.config
        if (Kq != 1 or I < 2 or select or masked or self.attn_fp8 or not self.fuse_bwd
                or K.matmul_mode() not in ('split', 'f32') or not K.last_fold()
                or not K.attn_fold_supported(cfg.hidden_dim, cfg.num_heads)):
            return None
        return self.fold_ded(I)

    def head_rows(self, B):
        key = ('head', B)
        if key not in self._aux_maps:
            self._aux_maps[key] = head_map(B, len(self.config.tasks))
        return self._aux_maps[key]

    def ident_rows(self, B):
        key = ('ident', B)
        if key not in self._aux_maps:
            self._aux_maps[key] = identity_map(B)
        return self._aux_maps[key]

    def single_group_chunks(self, mt_dev):
        """Chunks of a row map re-labelled as one group (Wo is shared by every position)."""
        key = ('single', mt_dev['chunks'].data_ptr())
        if key not in self._aux_maps:
            ch = mt_dev['chunks'].clone()
            ch[:, 0] = 0
            g = torch.tensor([[0, ch.shape[0]]], dtype=torch.int32, device=ch.device)
            self._aux_maps[key] = {'chunks': ch, 'gchunk': g}
        return self._aux_maps[key]

    # ---------------------------------------------------------------- input plan
    def _plan(self, ns: Dict[str, torch.Tensor], seq: Dict[str, torch.Tensor], training: bool = False):
        cfg = self.config
        d = cfg.hidden_dim
        dev = self.device
        B = next(iter(ns.values())).shape[0] if ns else next(iter(seq.values())).shape[0]
        seq_names = cfg.feature_config['sequence_features']
        present = [(i, n, int(seq[n].shape[1])) for i, n in enumerate(seq_names) if n in seq]
        ns_present = tuple(n for n in cfg.ns_feature_names() if n in ns)
        id_seq = bool(cfg.seq_item_vocab) and bool(present) and not torch.is_floating_point(torch.as_tensor(seq[present[0][1]]))
        bags = self._bag_inputs(ns, ns_present, B) if cfg.bag_features else ()
        key = (B, tuple(present), ns_present, id_seq) + ((tuple((n, cap, w is not None) for n, cap, _, w in bags),)
                                                         if bags else ())
        times = self._seq_times(seq, present, B) if self.time_fusion and present else None
        lens = self._seq_lengths(seq, present, B) if self.padding_mask else None
        plan = self._plans.get(key)
        if plan is None:
            plan = self._build_plan(B, present, ns_present, id_seq, bags)
            self._plans[key] = plan
        # ---- per-call data (copies into the plan's persistent buffers; no host sync)
        plan['gen'] += 1
        if plan['ns_fields'] > 0:
            if plan['n_dense'] > 0:
                plan['dense_buf'].copy_(torch.cat([ns[n].reshape(B, 1).to(dev, torch.float32)
                                                   for n in plan['dense_names']], 1))
            if plan['n_sparse'] > 0:
                plan['ids_buf'].copy_(torch.cat([ns[n].reshape(B, 1).to(dev, torch.int64)
                                                 for n in plan['sparse_names']], 1))
            for (n, cap, ids, w), (ids_buf, w_buf) in zip(bags, plan['bag_bufs']):
                ids_buf.copy_(ids)
                if w_buf is not None:
                    w_buf.copy_(w)
            for k, tname in enumerate(plan.get('bag_tables', ())):
                # (host descriptors: a table replaced since the plan was built, e.g. by load_weights, is followed)
                plan['bag_descs'][k].table = self.tables[tname].data_ptr()
        if plan['seq_map'] is not None:
            if self.time_fusion:
                # timestamp-aware fusion: stage the events' times and order each sample's events on the device;
                # the projection GEMM, its weight gradient and the embedding dgrad read the resulting x0 rows
                for buf, t in zip(plan['time_bufs'], times):
                    buf.copy_(t)
                K.seq_time_rows(plan['time_descs'], len(present), B, plan['L_S'], plan['L0'], plan['seq_rows_t'],
                                rank_out=plan['seq_rank'], last_time=plan['last_time'], device=dev)
            if self.padding_mask:
                self._stage_valid(plan, lens, B)
            if id_seq and 'emb.seq_item' in self.sharded:
                # row-sharded table: the rows arrive through the all-to-all lookup in token order, and
                # the projection reads them through the static (identity) row map; the ids are staged
                # and routed on the table's route stream (host ids copied there, device ids after
                # ``inputs_ready``), so its one host wait does not drain the main stream
                st = self.sharded['emb.seq_item']
                srcs = [seq[n] for (_, n, _) in present]
                ids = [s_ if isinstance(s_, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s_)) for s_ in srcs]
                # route_ahead() routed the next TRAINING forward's ids: only a training forward consumes it (an
                # evaluation forward in between routes its own ids), and it must be handed the very id objects
                # that were routed (PendingRoute.matches)
                routed = None
                if training and self._pending_route is not None:
                    routed, self._pending_route = self._pending_route, None
                plan['seq_A'] = st.lookup(ids, ready=self.inputs_ready, routed=routed, srcs=srcs)
                plan['seq_ids'] = st.last_ids
                plan['seq_route'] = st.last_route
            elif id_seq:
                ids = [seq[n].to(dev, torch.int64).contiguous() for (_, n, _) in present]
                for (i, n, L), t, off in zip(present, ids, plan['seq_seg_off']):
                    K.seq_rows(t, L, B, L, cfg.seq_item_vocab, (plan['seq_in'], off))
                plan['seq_ids'] = torch.cat([t.reshape(-1) for t in ids])
                # (a replicated table's ids: the optimizer builds the DP exchange's touched-row mask from them)
                self.last_table_ids = {'emb.seq_item': plan['seq_ids']}
                plan['seq_A'] = self.tables['emb.seq_item']
            else:
                buf = plan['seq_buf']
                o = 0
                for (i, n, L) in present:
                    buf[o:o + B * L].copy_(seq[n].reshape(B * L, -1).to(dev, torch.float32))
                    o += B * L
                plan['seq_A'] = buf
                plan['seq_ids'] = None
        if self.padding_mask and plan['seq_map'] is None:
            self._stage_valid(plan, [], B)             # no sequence present: every token is valid
        return plan

    def _seq_lengths(self, seq, present, B) -> List[torch.Tensor]:
        """The present sequences' real-event counts (``seq_padding_mask``): ``seq[name + seq_len_suffix]``, an integer
        [B] or [B, 1] host array or device tensor each.  A host array is range-checked here; a device tensor is not read
        back (ot_seq_key_valid clamps it)."""
        sfx = self.config.seq_len_suffix
        out = []
        for (_, n, L) in present:
            if n + sfx not in seq:
                raise ValueError(f'seq_padding_mask: sequence {n!r} has no lengths ({n + sfx!r} is missing from '
                                 'seq_features)')
            t = seq[n + sfx]
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
            if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
                raise TypeError(f'seq_padding_mask: the lengths of sequence {n!r} ({n + sfx!r}) are {t.dtype}; '
                                'integers are expected')
            if tuple(t.shape) not in ((B,), (B, 1)):
                raise ValueError(f'seq_padding_mask: the lengths of sequence {n!r} ({n + sfx!r}) have shape '
                                 f'{tuple(t.shape)}, expected {(B,)} or {(B, 1)}')
            if t.device.type == 'cpu' and B and (int(t.min()) < 0 or int(t.max()) > L):
                raise ValueError(f'seq_padding_mask: the lengths of sequence {n!r} ({n + sfx!r}) leave [0, {L}]')
            out.append(t.reshape(B))
        return out

    def _stage_valid(self, plan, lens, B) -> None:
        """Layer 0's key-padding mask of this call, plan['valid0'] [B, L0] uint8: the lengths staged into the plan's
        buffer, then one ot_seq_key_valid launch (after ot_seq_time_rows under time fusion: it reads the ranks).  A
        fresh array per call — the backward of this forward keeps reading it after a later forward restaged the plan."""
        dev = self.device
        groups = plan.get('seq_groups', []) if lens else []
        if lens:
            buf = plan['len_buf']
            for k, (t, (_, _, L)) in enumerate(zip(lens, groups)):
                buf[k].copy_(t.clamp(0, L))             # (before the narrowing to int32; no read-back)
        valid0 = torch.empty(B, plan['L0'], dtype=torch.uint8, device=dev)
        K.seq_key_valid(plan['len_buf'] if lens else None, [L for (_, _, L) in groups], [p0 for (_, p0, _) in groups],
                        B, plan['L0'], valid0, rank=plan.get('seq_rank') if lens else None)
        plan['valid0'] = valid0

    def _bag_inputs(self, ns, ns_present, B):
        """The present bag features' inputs as (name, cap, ids [B, cap], weights [B, cap] or None): integer ids, and
        optional float weights ``ns[name + '_weight']`` (pooling 'sum' only, as torch.nn.EmbeddingBag)."""
        cfg = self.config
        out = []
        for n in ns_present:
            if n not in cfg.bag_features:
                continue
            ids = ns[n]
            ids = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ids))
            if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
                raise TypeError(f'bag feature {n!r}: integer ids are expected, got {ids.dtype}')
            if ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1:
                raise ValueError(f'bag feature {n!r}: ids of shape [B, cap] with cap >= 1 are expected, got '
                                 f'{tuple(ids.shape)} (B = {B})')
            w = ns.get(n + '_weight')
            if w is not None:
                if cfg.bag_pooling(n) != 'sum':
                    raise ValueError(f"bag feature {n!r}: per-slot weights need pooling 'sum' (it is "
                                     f'{cfg.bag_pooling(n)!r})')
                w = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w))
                if tuple(w.shape) != tuple(ids.shape) or not w.is_floating_point():
                    raise ValueError(f'bag feature {n!r}: weights must be floats of the ids\' shape '
                                     f'{tuple(ids.shape)}, got {w.dtype} {tuple(w.shape)}')
            out.append((n, int(ids.shape[1]), ids, w))
        return tuple(out)

    def _seq_times(self, seq, present, B) -> List[torch.Tensor]:
        """The present sequences' event times (``seq_fusion='time'``): ``seq[name + seq_time_suffix]``, an integer
        [B, L_name] host array or device tensor each."""
        sfx = self.config.seq_time_suffix
        out = []
        for (_, n, L) in present:
            if n + sfx not in seq:
                raise ValueError(f"seq_fusion='time': sequence {n!r} has no times ({n + sfx!r} is missing from "
                                 'seq_features)')
            t = seq[n + sfx]
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
            if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
                raise TypeError(f'seq_fusion=\'time\': the times of sequence {n!r} ({n + sfx!r}) are {t.dtype}; '
                                'integer timestamps are expected (they are widened to int64)')
            if tuple(t.shape) != (B, L):
                raise ValueError(f"seq_fusion='time': the times of sequence {n!r} ({n + sfx!r}) have shape "
                                 f'{tuple(t.shape)}, expected {(B, L)}')
            out.append(t)
        return out

    def _build_plan(self, B, present, ns_present, id_seq, bags=()):
        cfg = self.config
        d = cfg.hidden_dim
        dev = self.device
        nseq_cfg = len(cfg.feature_config['sequence_features'])
        plan = {'B': B, 'gen': 0}
        if self.time_fusion and present and id_seq and 'emb.seq_item' in self.sharded:
            raise NotImplementedError("seq_fusion='time' with a row-sharded emb.seq_item table is not supported: the "
                                      "sharded lookup delivers rows through a static token-order route; use "
                                      "table_sharding='none' or seq_fusion='sep'")
        # ---- sequence token positions (model.py:259-277; 'time': the concatenation without [SEP] — the places
        # the events take when their times reproduce it; the per-call order comes from ot_seq_time_rows)
        pos = 0
        seq_groups, sep_pos = [], []
        for (i, n, L) in present:
            seq_groups.append((i, pos, L))
            pos += L
            if i < nseq_cfg - 1 and not self.time_fusion:
                sep_pos.append(pos)
                pos += 1
        L_S = pos
        L0 = L_S + cfg.num_ns_tokens
        plan.update(L_S=L_S, L0=L0, nseq=nseq_cfg)
        b = np.arange(B)
        if sep_pos:
            sep_rows = (b[:, None] * L0 + np.array(sep_pos)[None, :]).reshape(-1).astype(np.int32)
            plan['sep_rows'] = torch.from_numpy(sep_rows).to(dev)
        else:
            plan['sep_rows'] = None
        plan['n_sep'] = B * len(sep_pos)
        # ---- sequence projection GEMM maps: group = sequence index in the config
        if present:
            per_group = [[np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)]
                         for _ in range(nseq_cfg)]
            cmp_off = 0
            flat_off = 0
            for (i, p0, L) in seq_groups:
                m_ = np.arange(B * L)
                bb, pp = m_ // L, m_ % L
                per_group[i] = [bb * L0 + p0 + pp, cmp_off + m_, flat_off + m_]
                cmp_off += B * L
                flat_off += B * L
            rm = build_map(per_group)
            # rows[0]: x0 rows; rows[1]: compact rows (embedding-gradient output); rows[2]: float input rows
            plan['seq_map'] = rm
            plan['seq_M'] = cmp_off
            # segment offsets of each present sequence inside the padded map (for ot_seq_rows)
            offs = []
            starts = np.concatenate([[0], np.cumsum([round_up(len(pg[0]), TILE) for pg in per_group])])
            for (i, p0, L) in seq_groups:
                offs.append(int(starts[i]))
            plan['seq_seg_off'] = offs
            seq_in = torch.from_numpy(rm.rows[2].copy()).to(dev)
            plan['seq_in'] = seq_in
            if self.padding_mask:
                plan['seq_groups'] = seq_groups
                plan['len_buf'] = torch.zeros(len(seq_groups), B, dtype=torch.int32, device=dev)
            if not id_seq:
                plan['seq_buf'] = torch.empty(cmp_off, cfg.seq_feature_dim, device=dev)
            if self.time_fusion:
                if L_S > _lib.SEQ_TIME_MAX_L:
                    raise ValueError(f"seq_fusion='time': {L_S} events per sample, at most {_lib.SEQ_TIME_MAX_L}")
                # persistent per-call buffers (restaged by every _plan; the backward's generation guard covers
                # them): the times, the map's x0 rows (a copy of the static rows, whose -1 padding the kernel
                # never touches), each event's rank in concatenation order and the samples' latest time
                plan['time_bufs'] = [torch.empty(B, L, dtype=torch.int64, device=dev) for (_, _, L) in seq_groups]
                plan['time_descs'] = K.seq_time_descs([(t, L, L, off) for t, (_, _, L), off
                                                       in zip(plan['time_bufs'], seq_groups, offs)])
                plan['seq_rows_t'] = torch.from_numpy(rm.rows[0].copy()).to(dev)
                plan['seq_rank'] = torch.empty(B, L_S, dtype=torch.int32, device=dev)
                plan['last_time'] = torch.empty(B, dtype=torch.int64, device=dev)
        else:
            plan['seq_map'] = None
        # ---- NS fields (model.py:243-253)
        offs = ns_table_offsets(cfg)
        dense_names = [n for n in ns_present if n not in cfg.sparse_features and n not in cfg.bag_features]
        sparse_names = [n for n in ns_present if n in cfg.sparse_features]
        plan.update(dense_names=dense_names, sparse_names=sparse_names, n_dense=len(dense_names),
                    n_sparse=len(sparse_names), ns_fields=len(ns_present),
                    ns_desc_n=len(dense_names) + len(sparse_names), n_bags=0, n_bags_ns=0, bag_bufs=[],
                    bag_slots=0, bag_ns_slots=0)
        plan['nsmat'] = torch.zeros(B, self.layout.f_pad, device=dev)
        if ns_present:
            plan['dense_buf'] = torch.zeros(B, max(1, len(dense_names)), device=dev)
            plan['ids_buf'] = torch.zeros(B, max(1, len(sparse_names)), dtype=torch.int64, device=dev)
            # descriptors: sparse fields first (ot_ns_grad_pack packs the first n_sparse)
            if self.layout.ns_groups is not None:
                # group mode: every configured feature owns fixed columns inside its group's range (group-major,
                # following goff); a feature absent from the batch leaves its columns zero
                col = self.layout.ns_groups['col']
            else:
                col = {}
                c = 0
                for n in ns_present:
                    col[n] = c
                    c += cfg.ns_feature_width(n)
            recs = np.zeros(max(1, plan['ns_desc_n']),
                            dtype=np.dtype([('dense', '<u8'), ('ids', '<u8'), ('row_offset', '<i8'),
                                            ('stride', '<i8'), ('col', '<i4'), ('width', '<i4')]))
            assert recs.dtype.itemsize == NS_FIELD_BYTES
            k = 0
            for j, n in enumerate(sparse_names):
                recs[k] = (0, plan['ids_buf'].data_ptr() + 8 * j, offs[n], len(sparse_names), col[n],
                           cfg.ns_embedding_dim)
                k += 1
            for j, n in enumerate(dense_names):
                recs[k] = (plan['dense_buf'].data_ptr() + 4 * j, 0, 0, len(dense_names), col[n], 1)
                k += 1
            plan['ns_desc'] = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
            plan['ns_map'] = identity_map(B)
            if bags:
                self._plan_bags(plan, B, bags, col, offs)
        return plan

    def _plan_bags(self, plan, B, bags, col, offs) -> None:
        """The plan's bag features: persistent staging buffers for the ids (and weights), the host
        descriptors of ot_ns_bag_pool / ot_ns_bag_grad_pack — the emb.ns bags first, then the emb.seq_item bags,
        so each table's bags are one run of descriptors and of coefficient slots — and the coefficient buffer."""
        cfg, dev = self.config, self.device
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError('bag_features: data-parallel runs (world size > 1) are not supported (the '
                                      'sparse all-gather and the early dense exchange are not exercised with bags)')
        if len(bags) > _lib.NS_BAG_MAX:
            raise ValueError(f'bag_features: {len(bags)} bag features in one batch, at most {_lib.NS_BAG_MAX}')
        is_seq = lambda n: cfg.bag_features[n].get('table') == 'seq_item'
        if any(is_seq(n) for n, _, _, _ in bags) and 'emb.seq_item' in self.sharded:
            raise NotImplementedError("bag_features: a 'seq_item' bag with a row-sharded emb.seq_item table is not "
                                      "supported (the bag gathers local rows); use table_sharding='none'")
        order = sorted(range(len(bags)), key=lambda i: is_seq(bags[i][0]))          # stable: emb.ns bags first
        bufs = [None] * len(bags)
        recs = []
        for i in order:
            n, cap, _, w = bags[i]
            E = cfg.ns_feature_width(n)
            if E % 4 or E > _lib.NS_BAG_MAX_WIDTH:
                raise ValueError(f'bag feature {n!r}: row width {E} must be a multiple of 4, at most '
                                 f'{_lib.NS_BAG_MAX_WIDTH}')
            ids_buf = torch.full((B, cap), -1, dtype=torch.int64, device=dev)
            w_buf = torch.zeros(B, cap, device=dev) if w is not None else None
            bufs[i] = (ids_buf, w_buf)
            recs.append(dict(table=self.tables['emb.seq_item' if is_seq(n) else 'emb.ns'], ids=ids_buf, weights=w_buf,
                             row_offset=0 if is_seq(n) else offs[n], num_rows=cfg.bag_rows(n), ids_stride=cap,
                             weights_stride=cap, width=E, cap=cap, col=col[n], pooling=cfg.bag_pooling(n)))
        n_ns = sum(1 for i in order if not is_seq(bags[i][0]))
        slots = [B * r['cap'] for r in recs]
        plan.update(n_bags=len(bags), n_bags_ns=n_ns, bag_bufs=bufs, bag_slots=sum(slots),
                    bag_ns_slots=sum(slots[:n_ns]), bag_descs=K.ns_bag_descs(recs),
                    bag_tables=['emb.seq_item' if is_seq(bags[i][0]) else 'emb.ns' for i in order],
                    bag_coef=torch.zeros(max(1, sum(slots)), device=dev))

    # ---------------------------------------------------------------- forward
    def forward(self, non_seq_features, seq_features=None, training: bool = False,
                use_kv_cache: bool = False):
        """model.py:335-393.  Returns {task: probs [B, 1]} (sigmoid outputs, like the Keras heads).
        ``training`` defaults to False exactly like the reference signature (model.py:337), independent
        of nn.Module.train()/eval().  ``use_kv_cache`` is accepted for signature compatibility; the
        reference's cache path is defective (D6) and a full forward is computed."""
        if seq_features is None and isinstance(non_seq_features, (tuple, list)) and len(non_seq_features) == 2:
            non_seq_features, seq_features = non_seq_features           # D4: callers pass one tuple
        seq_features = seq_features or {}
        training = bool(training)
        probs = self.forward_probs(non_seq_features, seq_features, training)
        return {t: probs[i].view(-1, 1) for i, t in enumerate(self.config.tasks)}

    @in_model_precision
    def forward_probs(self, ns, seq, training: bool) -> torch.Tensor:
        """All tasks as one [T, B] tensor (the trainer's fused loss consumes it)."""
        plan = self._plan(ns, seq, training)
        bounds = PairBounds.begin(self.config.num_layers, self.device, K.matmul_mode(), self.pair_wgrad)
        seed = 0
        if training:
            self._step += 1
            seed = (self.dropout_seed + 0x9E3779B9 * self._step) & 0xFFFFFFFF
        x = _Tokenize.apply(self.flat, self, plan)
        sched = self.config.pyramid_schedule(plan['L0'])
        nl = len(sched)
        b0 = self.batch_offset(plan['B']) if training else 0
        rstd = None
        for l, s in enumerate(sched):
            Kq = s['keep'] if l < nl - 1 else 1
            select = l < nl - 1 and Kq < s['in_len']         # a pyramid keep (the last layer: DCE, tail)
            x, rstd = _Block.apply(self.flat, x, self, l, s['in_len'], Kq, layer_seed(seed, b0, s['in_len'],
                                   self.config.hidden_dim), training, rstd, select, bounds, plan.get('valid0'))
        probs, logits = _Head.apply(self.flat, x, self)
        probs._ot_logits = logits            # keras_bce_loss takes the BCE from the logits (Keras _keras_logits)
        return probs

    # ---------------------------------------------------------------- request-grouped forward
    def forward_requests(self, non_seq_features, seq_features, req, training: bool = False, validate: bool = True):
        """Request-grouped forward (paper §3.5.1 in training; recommend_amd/request_train.py): ``seq_features``
        hold R rows (one per request), ``non_seq_features`` C rows (one per candidate), ``req`` [C] integers,
        non-decreasing, in [0, R): the request of each candidate.  The S side of every layer runs once per
        request.  Returns {task: probs [C, 1]}, equal to ``forward`` on the expanded batch (each candidate with
        a copy of its request's sequences).  ``validate`` checks ``req`` with one small read-back before any
        launch (ValueError); with False the caller vouches for it."""
        probs = self.forward_probs_requests(non_seq_features, seq_features, req, bool(training), validate)
        return {t: probs[i].view(-1, 1) for i, t in enumerate(self.config.tasks)}

    @in_model_precision
    def forward_probs_requests(self, ns, seq, req, training: bool = False, validate: bool = True) -> torch.Tensor:
        """All tasks as one [T, C] tensor (``_ot_logits`` set, like ``forward_probs``)."""
        from . import request_train
        return request_train.forward_probs_requests(self, ns, seq, req, training, validate)

    def route_ahead(self, seq_features: Dict) -> None:
        """Look-ahead routing of the row-sharded item table (sharded.py ShardedTable.route): issue the routing of
        the NEXT forward's sequence ids now — the trainer calls it between step i's forward and backward with
        step i + 1's batch, so the split-size all-to-all and its host copy run beside step i's backward and the
        next lookup finds them done.  The next forward must be called with the same id tensors."""
        if 'emb.seq_item' not in self.sharded or not seq_features:
            return
        names = [n for n in self.config.feature_config['sequence_features'] if n in seq_features]
        if not names or torch.is_floating_point(torch.as_tensor(seq_features[names[0]])):
            return
        srcs = [seq_features[n] for n in names]
        ids = [s_ if isinstance(s_, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s_)) for s_ in srcs]
        self._pending_route = self.sharded['emb.seq_item'].route(ids, ready=self.inputs_ready, srcs=srcs)

    def batch_offset(self, B: int) -> int:
        """Index of this process's first sample in the global batch (dropout masks are a function of the
        global sample index, so a data-parallel step draws the masks of the equivalent full-batch step).
        ``sample_offset`` when set; else rank * B under torch.distributed (equal local batches)."""
        if self.sample_offset is not None:
            return int(self.sample_offset)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist.get_rank() * B
        return 0

    # ---------------------------------------------------------------- streams
    def comm_stream(self):
        """The communication stream: the dense gradient all-reduces (OneTransOptimizer) and the row-sharded
        tables' id routing share it, so a rank drives four hardware queues (GPU_MAX_HW_QUEUES = 4): the main
        stream, the weight-gradient side stream, this one and RCCL's internal stream."""
        if getattr(self, '_comm', None) is None:
            self._comm = torch.cuda.Stream(device=self.device)
        return self._comm

    # ---------------------------------------------------------------- side stream (wgrad overlap)
    def side(self, *tensors):
        """Context running the enclosed launches on the weight-gradient side stream, after the main
        stream's pending work.  ``tensors`` (inputs produced on the main stream) are kept referenced
        until ``join_side_stream`` has made the main stream wait for the side stream, so the caching
        allocator cannot hand their memory to a main-stream allocation while a side kernel still reads
        it.  (``record_stream`` would do the same but defers frees behind events, which makes the
        allocator grow with fresh device allocations step after step.)"""
        import contextlib
        if not self.overlap_wgrad:
            return contextlib.nullcontext()
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(main)
        self._side_keep.extend(tensors)
        self._side_used = True
        return torch.cuda.stream(self._side)

    def side_block_done(self, depth: int = 2):
        """End of one block's backward: the tensors its side-stream launches read are released once the
        side stream has finished them — the main stream waits on an event recorded after the block's
        weight gradients, ``depth`` blocks later (by then the side stream has normally finished them, so
        nothing stalls), instead of holding every block's backward temporaries until the join."""
        if self._side is None or not self._side_keep:
            return
        ev = torch.cuda.Event()
        ev.record(self._side)
        self._side_fifo.append((ev, self._side_keep))
        self._side_keep = []
        while len(self._side_fifo) > depth:
            ev0, _ = self._side_fifo.pop(0)
            torch.cuda.current_stream(self.device).wait_event(ev0)

    def join_side_stream(self):
        """The main stream waits for every weight gradient launched on the side stream."""
        if self._side is not None and self._side_used:
            torch.cuda.current_stream(self.device).wait_stream(self._side)
            self._side_used = False
        self._side_keep = []
        self._side_fifo = []

    # ---------------------------------------------------------------- reference API
    def reset_kv_cache(self):
        """model.py:395-397."""
        self.kv_cache = None

    def get_model_info(self) -> Dict:
        """model.py:399-408 (count of the reference's trainable weights; embedding tables of the
        build extension reported separately)."""
        n = int(sum(r * c for (_, r, c, _) in self.layout.segments))
        return {'total_parameters': n, 'num_layers': self.config.num_layers,
                'hidden_dim': self.config.hidden_dim, 'num_heads': self.config.num_heads,
                'embedding_rows': {k: int(v.shape[0]) for k, v in self.tables.items()}}

    def save_weights(self, path: str) -> None:
        """Counterpart of model.save_weights (train.py:286): one .npz of named banks.  Collective when a
        table is row-sharded (every rank calls it; the gathered table is written by rank 0 only)."""
        params = self.param_dict()
        if self.layout.ns_groups is not None:                 # which feature owns which rows of tok.ns.kernel
            params[NS_GROUPS_KEY] = np.array(json.dumps(self.layout.ns_groups['members']))
        if self.sharded and self._rank() != 0:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.savez(path, **params)

    @staticmethod
    def _rank() -> int:
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def load_weights(self, path: str) -> None:
        """Counterpart of model.load_weights (train.py:332)."""
        with np.load(path, allow_pickle=False) as z:
            params = {k: z[k] for k in z.files}
        saved = params.pop(NS_GROUPS_KEY, None)
        mine = self.layout.ns_groups['members'] if self.layout.ns_groups is not None else None
        saved = json.loads(str(saved)) if saved is not None else None
        if saved != mine:
            raise ValueError(f'{path}: the weights were saved with '
                             + ("ns_tokenizer='auto'" if saved is None else f"ns_tokenizer='group', groups {saved}")
                             + ', this model has '
                             + ("ns_tokenizer='auto'" if mine is None else f"ns_tokenizer='group', groups {mine}"))
        self.load_param_dict(params)


def create_onetrans_model(model_type: str = 'default', device=None) -> OneTransModel:
    """model.py:411-416."""
    return OneTransModel(get_model_config(model_type), device=device)
