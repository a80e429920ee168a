"""OneTransTrainer — mirrors the reference trainer (``practice/train.py:19-374``).

``train_step`` is the metric's "fwd+bwd" unit (train.py:111-155): forward (tuple call
convention, train.py:118) -> Σ_task Keras BCE (train.py:124-128) -> backward (train.py:131) ->
per-variable clip_by_norm (train.py:134-135) -> RMSprop(momentum) or Adam, whichever
``optimizer_config['dense_optimizer']`` selects (train.py:53-76, 138) -> sparse Adagrad
on the embedding rows touched (build extension), with one accumulator per element or, under
``optimizer_config['sparse_optimizer'] = 'rowwise_adagrad'``, per row.  Defect D5 mapping: the trainer reads
``gradient_clip_norm`` (the reference reads the absent ``gradient_clip``) and
``optimizer_config['dense_lr']`` (the reference reads the absent ``learning_rate``); mixed
precision is not enabled (the reference reads the absent ``system_config``) — the HIP path
computes in fp32 like the Keras default policy.
"""

from __future__ import annotations

import json
import os
import time
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import dist as otdist
from . import kernels as K
from .config import (LOSS_WEIGHT_MAX, OneTransConfig, dense_optimizer_spec, get_model_config, sparse_optimizer_spec,
                     task_loss_scale)
from .loss import BINARY_TASKS, keras_bce_loss
from .metrics import GroupedAUC, StreamingMetrics, auc, div_no_nan, keras_auc
from .model import OneTransModel


def _to_dev(d: Dict, dev) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in d.items():
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        out[k] = t.to(dev, non_blocking=True)
    return out


def _seq_inputs(model, seq: Dict, dev) -> Dict:
    """Sequence features for forward_probs: with a row-sharded item table the id sequences stay as the caller
    gave them (host arrays or tensors) — the lookup copies them on the table's route stream, off the main stream
    (sharded.py), and a look-ahead route (route_ahead) is matched against these very objects."""
    if not getattr(model, 'sharded', None):
        return _to_dev(seq, dev)
    return dict(seq)


def _split_batch(batch_data):
    """(non_seq, seq, labels, req): a 3-tuple batch has req None; a 4-tuple is request-grouped
    (data.make_request_batch: sequences per request, ``req`` [C] the request of each candidate)."""
    if len(batch_data) == 4:
        return batch_data
    non_seq, seq, labels = batch_data
    return non_seq, seq, labels, None


def label_rank(labels, tasks=None) -> int:
    """Rank of the caller's per-task labels: 1 for [B] (get_tf_dataset's batched scalars), 2 for [B, 1]
    (create_sample_batch) and for an already stacked [T, B] tensor.  It picks the BCE form (keras_bce_loss).
    ``tasks``: look at these keys only (a weighted batch carries weight arrays beside the labels)."""
    if isinstance(labels, torch.Tensor):
        return 2
    return min(2, max(np.ndim(v) for k, v in labels.items() if tasks is None or k in tasks))


def stack_labels(labels: Dict, tasks, dev) -> torch.Tensor:
    """{task: [B,1]} -> [T, B] float32 on device."""
    return torch.stack([torch.as_tensor(labels[t]).reshape(-1).to(dev, torch.float32) for t in tasks])


def _weight_row(v, name: str, B: int, dev) -> torch.Tensor:
    """One weight array ([B] or [B, 1]) as a [B] float32 device tensor.  A host array is checked here (NaN, negative
    or above the range: ValueError before any launch); a device tensor is never read back (the kernels clamp it)."""
    if isinstance(v, torch.Tensor) and v.device.type != 'cpu':
        if not v.is_floating_point():
            raise ValueError(f'labels[{name!r}]: a floating-point weight expected, got {v.dtype}')
        t = v
    else:
        a = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if a.dtype.kind != 'f':
            raise ValueError(f'labels[{name!r}]: a floating-point weight expected, got {a.dtype}')
        if not bool(np.all((a >= 0) & (a <= LOSS_WEIGHT_MAX))):          # (a NaN fails both compares)
            raise ValueError(f'labels[{name!r}]: weights must lie in [0, {int(LOSS_WEIGHT_MAX)}] (no NaN)')
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.numel() != B or t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1):
        raise ValueError(f'labels[{name!r}]: shape {tuple(t.shape)}; expected [{B}] or [{B}, 1]')
    return t.reshape(-1).to(dev, torch.float32)


def stack_weights(labels: Dict, config: OneTransConfig, dev) -> Optional[torch.Tensor]:
    """The [T, B] float32 weights of a batch, w[t, b] = sample_weight[b] * task_weight_t[b], from
    ``labels[config.sample_weight_key]`` and ``labels[task + config.label_weight_suffix]`` (each [B] or [B, 1]
    floating point, a host array or a device tensor; a missing factor is 1), or None when the batch carries
    neither.  With only a sample weight the result is one row expanded over the tasks (stride 0).  The product of two
    in-range factors may leave the range: the kernels clamp it."""
    if isinstance(labels, torch.Tensor):
        return None
    tasks = list(config.tasks)
    sw_key, suf = config.sample_weight_key, config.label_weight_suffix
    present = [k for k in [sw_key] + [t + suf for t in tasks] if k in labels]
    if not present:
        return None
    B = int(np.prod(np.shape(labels[tasks[0]])))
    sw = _weight_row(labels[sw_key], sw_key, B, dev) if sw_key in labels else None
    if all(t + suf not in labels for t in tasks):
        return sw.unsqueeze(0).expand(len(tasks), B)
    rows = []
    for t in tasks:
        tw = _weight_row(labels[t + suf], t + suf, B, dev) if t + suf in labels else None
        if tw is None:
            rows.append(sw if sw is not None else torch.ones(B, dtype=torch.float32, device=dev))
        else:
            rows.append(tw * sw if sw is not None else tw)
    return torch.stack(rows)


class OneTransOptimizer:
    """Dense: clip_by_norm per reference variable + the optimizer ``optimizer_config['dense_optimizer']`` names
    (config.dense_optimizer_spec, train.py:53-76) on the flat buffer, one fused multi-segment call: Keras
    RMSprop(momentum) (ot_clip_rmsprop) or Keras Adam (ot_clip_adam).  Both keep two flat state buffers: ``v`` and
    ``m`` (RMSprop: mean square and momentum; Adam: second and first moment).  Sparse: the optimizer
    ``optimizer_config['sparse_optimizer']`` names (config.sparse_optimizer_spec) on the de-duplicated rows of each
    embedding table: Keras Adagrad with one accumulator per element (``'adagrad'``, ot_sparse_adagrad; ``acc[name]``
    is shaped like the table) or per row (``'rowwise_adagrad'``, ot_sparse_adagrad_rowwise; ``acc[name]`` is [rows],
    for a row-sharded table one entry per allocated shard row)."""

    def __init__(self, model: OneTransModel, config: OneTransConfig):
        self.model = model
        oc = config.optimizer_config
        self.kind, spec = dense_optimizer_spec(config)
        self.lr = spec['lr']
        # linear warm-up of the dense learning rate over config.warmup_steps (config.py:36; the
        # reference defines warmup_steps but never applies it, so this is opt-in: apply_warmup)
        self.warmup = int(config.warmup_steps) if getattr(config, 'apply_warmup', False) else 0
        self.steps_done = 0
        self.eps = spec['eps']
        if self.kind == 'rmsprop':
            self.momentum, self.rho = spec['momentum'], spec['rho']
        else:
            self.beta1, self.beta2 = spec['beta1'], spec['beta2']
        self.clip = float(config.gradient_clip_norm)
        self.sparse_kind, sspec = sparse_optimizer_spec(config)      # (an unknown name: ValueError)
        self.sparse_lr, self.sparse_eps, self.sparse_clip = sspec['lr'], sspec['eps'], sspec['clip']
        dev = model.flat.device
        self.v = torch.zeros_like(model.flat.data)
        self.m = torch.zeros_like(model.flat.data)
        self.segs = torch.from_numpy(model.layout.segments.reshape(-1)).to(dev)
        self.nseg = model.layout.segments.shape[0]
        if self.sparse_kind == 'rowwise_adagrad':
            self.acc = {k: torch.full((t.shape[0],), sspec['initial_accumulator'], dtype=torch.float32,
                                      device=t.device) for k, t in model.tables.items()}
        else:
            self.acc = {k: torch.full_like(t, sspec['initial_accumulator']) for k, t in model.tables.items()}
        # data-parallel exchange of replicated tables: dense all-reduce up to this size, else all-gather
        self.dense_exchange_bytes = int(float(os.environ.get('ONETRANS_DENSE_EXCHANGE_MB', '512')) * 2 ** 20)
        # ... and of those, all-reduce only the rows some rank touched (the union, from a 1-byte-per-row
        # max all-reduce) when it is under 60% of a >= 128 MB table ('auto'), always ('1') or never ('0')
        self.compact_exchange = os.environ.get('ONETRANS_COMPACT_EXCHANGE', 'auto')
        self._dense_grad: Dict[str, torch.Tensor] = {}
        self._mask_buf: Dict[str, torch.Tensor] = {}
        self._masks: Dict = {}
        self._mask_stream = None
        self._mask_count: Dict[str, torch.Tensor] = {}
        # diagnostics (bench.py, N > 1): when a list, every step appends HIP-event pairs bracketing the
        # main stream's waits for the gradient exchange, i.e. the exchange time NOT hidden by backward
        self.exchange_events = None

    def current_lr(self) -> float:
        """Dense learning rate of the step being applied (``steps_done`` counts it): lr * min(1, step /
        warmup_steps) under ``apply_warmup``, else lr."""
        if self.warmup > 0:
            return self.lr * min(1.0, self.steps_done / self.warmup)
        return self.lr

    # ---------------------------------------------------------------- resumable state
    def state_dict(self) -> Dict[str, np.ndarray]:
        """Host copies of what a resumed run needs besides the weights: the dense kind, ``steps_done`` (Adam's bias
        correction and the warm-up ramp), the two flat dense slots and every table's Adagrad accumulator
        (``acc.<table>``: shaped like the table, or [rows] under ``'rowwise_adagrad'``).  ``'sparse_kind'`` names
        the table optimizer when it is not ``'adagrad'``: an ``'adagrad'`` state keeps the keys it always had, and a
        state without the key is an ``'adagrad'`` one.  Like ``OneTransModel.param_dict``, a COLLECTIVE with a
        row-sharded table (its accumulator is all-gathered into the logical table's row order): every rank calls
        it."""
        out = {'dense_kind': np.array(self.kind), 'steps_done': np.array(self.steps_done, dtype=np.int64),
               'dense.v': self.v.detach().cpu().numpy().copy(), 'dense.m': self.m.detach().cpu().numpy().copy()}
        if self.sparse_kind != 'adagrad':
            out['sparse_kind'] = np.array(self.sparse_kind)
        for name, a in self.acc.items():
            sh = self.model.sharded.get(name)
            src = sh.full_table(a) if sh is not None else a
            out[f'acc.{name}'] = src.detach().cpu().numpy().copy()
        return out

    def load_state_dict(self, d: Dict[str, np.ndarray]) -> None:
        """Restore ``state_dict()``'s arrays.  Everything is checked before anything is written: a state of the
        other dense or sparse kind (a state without ``'sparse_kind'``, written before there was a choice, counts as
        ``'adagrad'``), a missing entry or a shape that does not fit raises ValueError and leaves the optimizer as
        it was.  A row-sharded table's accumulator keeps this rank's rows (id % world == rank)."""
        kind = str(np.asarray(d['dense_kind']))
        if kind != self.kind:
            raise ValueError(f'optimizer state is for dense optimizer {kind!r}, this optimizer runs {self.kind!r}')
        skind = str(np.asarray(d['sparse_kind'])) if 'sparse_kind' in d else 'adagrad'
        if skind != self.sparse_kind:
            raise ValueError(f'optimizer state is for sparse optimizer {skind!r}, this optimizer runs '
                             f'{self.sparse_kind!r}')
        todo = []
        for key, dst in (('dense.v', self.v), ('dense.m', self.m)):
            todo.append((key, dst, np.asarray(d[key]) if key in d else None))
        for name, a in self.acc.items():
            key = f'acc.{name}'
            arr = np.asarray(d[key]) if key in d else None
            sh = self.model.sharded.get(name)
            if sh is not None:
                full = (sh.num_rows,) if self.sparse_kind == 'rowwise_adagrad' else (sh.num_rows, sh.E)
                if arr is not None and arr.shape != full:
                    raise ValueError(f'{key}: stored shape {arr.shape} != {full}')
                todo.append((key, a[:sh.local_rows], None if arr is None else arr[sh.rank::sh.world]))
            else:
                todo.append((key, a, arr))
        for key, dst, arr in todo:
            if arr is None:
                raise ValueError(f'optimizer state lacks {key!r}')
            if tuple(arr.shape) != tuple(dst.shape):
                raise ValueError(f'{key}: stored shape {tuple(arr.shape)} != {tuple(dst.shape)}')
        for key, dst, arr in todo:
            dst.copy_(torch.as_tensor(np.ascontiguousarray(arr), dtype=torch.float32))
        self.steps_done = int(np.asarray(d['steps_done']))

    def state_nbytes(self) -> int:
        """Device bytes of the optimizer state on this rank: the two flat dense slots plus every table's
        accumulator (a row-sharded table: this rank's shard)."""
        return sum(t.numel() * t.element_size() for t in (self.v, self.m, *self.acc.values()))

    def _mark(self):
        if self.exchange_events is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def exposed_exchange_ms(self) -> float:
        """Sum over the recorded steps of the exposed exchange time (ms); clears the record."""
        if not self.exchange_events:
            return 0.0
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for (a, b) in self.exchange_events)
        self.exchange_events = []
        return ms

    # ---------------------------------------------------------------- DP exchange overlapped with backward
    def bank_ranges(self):
        """Flat-buffer ranges that become final together in backward: 'head' (out_norm + heads), each
        block l, and the tokenizer remainder (layout order: tok.*, blk.0 .. blk.L-1, out_norm, head.*)."""
        lay, cfg = self.model.layout, self.model.config
        off = lay.offsets
        starts = [off[f'blk.{l}.norm1'] for l in range(cfg.num_layers)] + [off['out_norm']]
        r = {l: (starts[l], starts[l + 1]) for l in range(cfg.num_layers)}
        r['head'] = (off['out_norm'], lay.total)
        r['tok'] = (0, starts[0])
        return r

    def begin_backward(self) -> None:
        """Arm the per-bank all-reduce hooks for the next backward (world > 1, no accumulation): each
        block's gradient range is all-reduced on a communication stream as soon as its dgrad chain and
        its side-stream weight gradients are issued, overlapping the earlier layers' backward."""
        m = self.model
        if otdist.world() == 1 or m.accumulate_grads:
            m.grad_ready = None
            return
        if not hasattr(self, '_ranges'):
            self._ranges = self.bank_ranges()
            self._comm = m.comm_stream()
        self._works = []
        m.grad_ready = self._launch

    def _launch(self, key) -> None:
        m = self.model
        lo, hi = self._ranges[key]
        self._comm.wait_stream(torch.cuda.current_stream(m.flat.device))
        if m._side is not None:
            self._comm.wait_stream(m._side)              # this block's wgrads run on the side stream
        with torch.cuda.stream(self._comm):
            for s0 in range(lo, hi, otdist.BUCKET_ELEMS):          # 32 MiB buckets (one for a C2 block)
                self._works.append(otdist.allreduce_sum_async(m.flat.grad[s0:min(hi, s0 + otdist.BUCKET_ELEMS)]))

    def _compact(self, table: torch.Tensor) -> bool:
        """Exchange this replicated table's gradient as the union of touched rows (ONETRANS_COMPACT_EXCHANGE: '1'
        always, 'auto' for tables of >= 128 MB — each compaction costs a mask all-reduce and a host sync)?"""
        return self.compact_exchange == '1' or (self.compact_exchange == 'auto' and table.numel() * 4 >= 2 ** 27)

    def prepare_table_exchange(self) -> None:
        """Between the forward and the backward (OneTransTrainer.train_step): for each replicated table exchanged
        as the union of touched rows, build this rank's touched-row mask from the forward's ids, MAX-all-reduce it
        and count the union, all on a stream of its own that depends on the forward only; the count goes to pinned
        host memory.  step() then waits for that stream's event — long complete by the time the host has issued the
        backward — and takes the union's rows with ``torch.nonzero_static`` (no device sync), so the optimizer
        step has no host gap (the mask used to be built, reduced and ``torch.nonzero``-ed in step(), a sync on the
        whole queued backward)."""
        m = self.model
        self._masks = {}
        if otdist.world() == 1:
            return
        import torch.distributed as dist
        for name, ids in getattr(m, 'last_table_ids', {}).items():
            table = m.tables.get(name)
            if (ids is None or table is None or name in m.sharded or table.numel() * 4 > self.dense_exchange_bytes
                    or not self._compact(table)):
                continue
            rows = table.shape[0]
            mask = self._mask_buf.get(name)
            if mask is None:
                mask = self._mask_buf[name] = torch.zeros(rows, dtype=torch.uint8, device=table.device)
            if self._mask_stream is None:
                self._mask_stream = torch.cuda.Stream(device=table.device)
            cnt = self._mask_count.get(name)
            if cnt is None:
                cnt = self._mask_count[name] = torch.zeros(1, dtype=torch.int64, pin_memory=True)
            ms = self._mask_stream
            ms.wait_stream(torch.cuda.current_stream(table.device))      # the forward staged the ids
            with torch.cuda.stream(ms):
                mask.zero_()
                k = ids.reshape(-1)
                mask[k[(k >= 0) & (k < rows)]] = 1
                work = dist.all_reduce(mask, op=dist.ReduceOp.MAX, async_op=True)
                if dist.get_backend() == 'gloo':
                    # (the CPU rehearsal: gloo's wait blocks the host, so it and the count wait for step())
                    self._masks[name] = (mask, work, None)
                    continue
                work.wait()                              # RCCL: a stream dependency, no host wait
                cnt.copy_(torch.count_nonzero(mask).reshape(1), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(ms)
            self._masks[name] = (mask, None, ev)

    def _start_table_exchange(self, g: torch.Tensor, keys: torch.Tensor, name: str = None):
        """Start the sum over ranks of a replicated table's dense gradient ``g``.  C2's 1M-row item table
        is 256 MB, but a rank's batch touches ~1/6 of its rows: the ranks first agree on the union of
        touched rows (uint8 mask, max all-reduce, 1 B per row) and all-reduce only those rows
        (``ONETRANS_COMPACT_EXCHANGE``).  Rows outside the union are zero on every rank, so the result
        is the dense all-reduce's.  Returns (g, work, union rows or None, compact rows or None)."""
        import torch.distributed as dist
        rows = g.shape[0]
        if self._compact(g):
            pending = self._masks.pop(name, None) if name is not None else None
            if pending is not None:                      # built from the forward's ids, reduced during the backward
                mask, work, ev = pending
                if work is not None:                     # gloo: wait and count here
                    work.wait()
                    torch.cuda.current_stream(g.device).wait_stream(self._mask_stream)
                    idx = torch.nonzero(mask).reshape(-1)
                else:
                    ev.synchronize()                     # (the mask stream's work, not the queued backward)
                    torch.cuda.current_stream(g.device).wait_event(ev)
                    idx = torch.nonzero_static(mask, size=int(self._mask_count[name].item())).reshape(-1)
            else:
                mask = torch.zeros(rows, dtype=torch.uint8, device=g.device)
                k = keys.reshape(-1)
                mask[k[(k >= 0) & (k < rows)]] = 1
                dist.all_reduce(mask, op=dist.ReduceOp.MAX)
                idx = torch.nonzero(mask).reshape(-1)    # host sync: the union's size
            if self.compact_exchange == '1' or idx.numel() < 0.6 * rows:
                cg = g.index_select(0, idx)
                return g, otdist.allreduce_sum_async(cg), idx, cg
        return g, otdist.allreduce_sum_async(g), None, None

    @staticmethod
    def _join_pending(pending):
        """One (keys, grads) per table: entries naming the same table (a 'seq_item' bag next to the S sequences; the
        two plans of a request-grouped step) are concatenated, so the table gets one de-duplicated gradient, one
        clip and one Adagrad application.  A table with a single entry keeps its tensors as they are."""
        names = [name for (name, _, _) in pending]
        if len(set(names)) == len(names):
            return pending
        out = []
        for name in dict.fromkeys(names):
            ent = [(k, g) for (n, k, g) in pending if n == name]
            if len(ent) == 1:
                out.append((name, ent[0][0], ent[0][1]))
            else:
                out.append((name, torch.cat([k.reshape(-1) for k, _ in ent]),
                            torch.cat([g.reshape(-1, g.shape[-1]) for _, g in ent])))
        return out

    def step(self) -> None:
        m = self.model
        m._pending_sparse = self._join_pending(m._pending_sparse)
        # replicated tables small enough to exchange densely: scatter the de-duplicated gradient and
        # start its all-reduce first, so the dense optimizer below runs while it is in flight
        early = {}
        ev_a = self._mark() if otdist.world() > 1 else None
        if otdist.world() > 1:
            for (name, keys, grads) in m._pending_sparse:
                table = m.tables[name]
                if name in m.sharded or table.numel() * 4 > self.dense_exchange_bytes:
                    continue
                rows, E = table.shape
                g = self._dense_grad.get(name)
                if g is None:
                    g = self._dense_grad[name] = torch.zeros_like(table)
                else:
                    g.zero_()
                K.sparse_grad_dense(E, rows, keys, grads, keys.numel(), g, device=table.device)
                early[name] = self._start_table_exchange(g, keys, name)
        if m.grad_ready is not None:
            for w in self._works:                        # the current stream waits for each exchange
                w.wait()
            lo, hi = self._ranges['tok']
            otdist.allreduce_dense(m.flat.grad[lo:hi], scale=False)
            m.flat.grad.mul_(1.0 / otdist.world())
            m.grad_ready = None
            self._works = []
        else:
            otdist.allreduce_dense(m.flat.grad)
        if ev_a is not None:
            self.exchange_events.append((ev_a, self._mark()))
        self.steps_done += 1
        if self.kind == 'rmsprop':
            K.clip_rmsprop(m.flat.data, m.flat.grad, self.v, self.m, self.segs, self.nseg, m.layout.max_seg_elems,
                           self.current_lr(), self.rho, self.eps, self.momentum, self.clip, device=m.flat.device)
        else:
            K.clip_adam(m.flat.data, m.flat.grad, self.m, self.v, self.segs, self.nseg, m.layout.max_seg_elems,
                        self.current_lr(), self.beta1, self.beta2, self.eps, self.steps_done, self.clip,
                        device=m.flat.device)
        m.refresh_shadow()
        rowwise = self.sparse_kind == 'rowwise_adagrad'
        for (name, keys, grads) in m._pending_sparse:
            table = m.tables[name]
            rows, E = table.shape
            if name in m.sharded:
                # row-sharded: gradient rows go to their owners (all-to-all), global-norm clip, Adagrad
                m.sharded[name].apply_gradient(keys, grads, self.acc[name], self.sparse_lr, self.sparse_eps,
                                               self.sparse_clip, kind=self.sparse_kind)
            elif name in early:
                # one all-reduce of the de-duplicated dense gradient (started above) instead of
                # all-gathering every rank's rows
                g, work, idx, cg = early[name]
                ev_c = self._mark()
                work.wait()
                if ev_c is not None:
                    self.exchange_events.append((ev_c, self._mark()))
                if idx is not None:                      # the union's summed rows back into the dense gradient
                    g.index_copy_(0, idx, cg)
                g.mul_(1.0 / otdist.world())
                dense_update = K.dense_adagrad_rowwise if rowwise else K.dense_adagrad
                dense_update(table, self.acc[name], g, rows, E, self.sparse_lr, self.sparse_eps, self.sparse_clip,
                             device=table.device)
            else:
                keys, grads = otdist.allgather_sparse(keys, grads)
                sparse_update = K.sparse_adagrad_rowwise if rowwise else K.sparse_adagrad
                sparse_update(table, self.acc[name], E, rows, keys, grads, keys.numel(), self.sparse_lr,
                              self.sparse_eps, self.sparse_clip, device=table.device)
        m._pending_sparse = []


class OneTransTrainer:
    """train.py:19-338 surface: train_step / val_step / train / save_model / load_model."""

    def __init__(self, config: OneTransConfig, model_dir: str = './models', device=None,
                 model: Optional[OneTransModel] = None, seed: int = 0):
        self.config = config
        self.model_dir = Path(model_dir)
        self.model = model if model is not None else OneTransModel(config, device=device, seed=seed)
        self.device = self.model.flat.device
        self.optimizer = OneTransOptimizer(self.model, config)
        self.history = {'train_loss': [], 'val_loss': [], 'train_metrics': {}, 'val_metrics': {}}
        # the reference's running per-step metrics (train.py:95-109), off unless enable_metrics() / fit()
        self.train_metrics: Optional[StreamingMetrics] = None
        self.val_metrics: Optional[StreamingMetrics] = None
        # the paper's user-level AUC (metrics.GroupedAUC), off unless enable_metrics(group_feature=...)
        self.group_feature: Optional[str] = None
        self.train_grouped: Optional[GroupedAUC] = None
        self.val_grouped: Optional[GroupedAUC] = None

    def enable_metrics(self, num_thresholds: int = 200, group_feature: Optional[str] = None) -> None:
        """Create the running train / validation metric states (train.py:53-54, 95-109): from here on every
        ``train_step`` / ``val_step`` adds its batch to them with one stream-ordered launch (no host sync; the
        weights do not depend on it).  Off by default: the steps then launch exactly what they always did.
        ``group_feature`` (for example ``'user_id'``): the steps also log ``non_seq[group_feature]`` with the batch's
        labels and probabilities (metrics.GroupedAUC), and ``metric_results`` reports ``{t}_uauc*`` as well."""
        wl = bool(getattr(self.config, 'weighted_loss', False))      # the states then count in weight units
        self.train_metrics = StreamingMetrics(self.config.tasks, self.device, num_thresholds, weighted=wl)
        self.val_metrics = StreamingMetrics(self.config.tasks, self.device, num_thresholds, weighted=wl)
        self.group_feature = group_feature
        self.train_grouped = self.val_grouped = None
        if group_feature is not None:
            self.train_grouped = GroupedAUC(self.config.tasks, self.device)
            self.val_grouped = GroupedAUC(self.config.tasks, self.device)

    def metric_results(self, metrics: StreamingMetrics, extended: bool = False) -> Dict[str, float]:
        """``metrics.result()`` over all ranks: in a data-parallel run the state is summed over the ranks first
        (in place, as Keras aggregates metric variables under a distribution strategy).  With a group feature the
        grouped results of the same split are merged in (the records gathered from all ranks first)."""
        if otdist.world() > 1:
            metrics.all_reduce()
        res = metrics.result(extended)
        grouped = (getattr(self, 'train_grouped', None) if metrics is self.train_metrics else
                   getattr(self, 'val_grouped', None) if metrics is self.val_metrics else None)
        if grouped is not None:
            if otdist.world() > 1:
                grouped.all_gather()
            res.update(grouped.result())
        return res

    def _group_ids(self, non_seq) -> torch.Tensor:
        if self.group_feature not in non_seq:
            raise KeyError(f'enable_metrics(group_feature={self.group_feature!r}): the batch has no non-sequence '
                           f'feature of that name (it has {sorted(non_seq)})')
        return torch.as_tensor(non_seq[self.group_feature]).reshape(-1).to(self.device, torch.int64)

    def _weights(self, labels, grouped) -> Optional[torch.Tensor]:
        """``stack_weights`` of the batch under ``config.weighted_loss`` (None with the switch off: no key is
        read).  The grouped AUC stays un-weighted, so a weighted batch while a group feature is logged is refused."""
        if not getattr(self.config, 'weighted_loss', False):
            return None
        w = stack_weights(labels, self.config, self.device)
        if w is not None and grouped is not None:
            raise NotImplementedError('weighted_loss with enable_metrics(group_feature=...): the grouped AUC (UAUC) '
                                      'carries no sample weights; drop the weight keys or the group feature')
        return w

    def _loss(self, y, probs, labels, w) -> torch.Tensor:
        if not getattr(self.config, 'weighted_loss', False):
            # (the rank of the task labels alone: a weight array beside them is inert with the switch off)
            return keras_bce_loss(y, probs, self.config.tasks, label_rank(labels, self.config.tasks))
        if w is None:                                    # no weight key in this batch: every weight is 1
            w = torch.ones(y.shape[1], dtype=torch.float32, device=y.device)
        scale = task_loss_scale(self.config)
        if scale is not None:                            # the coefficients as a device tensor, uploaded once
            cached = getattr(self, '_task_scale', None)
            if cached is None or cached[0] != scale:
                cached = self._task_scale = (scale, torch.tensor(scale, dtype=torch.float32, device=y.device))
            scale = cached[1]
        return keras_bce_loss(y, probs, self.config.tasks, label_rank(labels, self.config.tasks), weights=w,
                              task_scale=scale, reduction=self.config.loss_reduction)

    @staticmethod
    def _update_metrics(metrics: StreamingMetrics, y, probs, w) -> None:
        if metrics.weighted:
            metrics.update(y, probs, weights=w)
        elif w is not None:
            raise ValueError('the running metrics were created with config.weighted_loss off; call enable_metrics() '
                             'again after switching it on')
        else:
            metrics.update(y, probs)

    # --------------------------------------------------------------- steps
    def train_step(self, batch_data, next_batch=None) -> Dict[str, torch.Tensor]:
        """train.py:111-155.  Returns {'total_loss': device scalar} (no host sync).  ``next_batch`` (optional, the
        batch the next call will get, e.g. from a prefetching loader): a row-sharded table routes its ids during
        this step (OneTransModel.route_ahead)."""
        non_seq, seq, labels, req = _split_batch(batch_data)
        dev = self.device
        y = labels if isinstance(labels, torch.Tensor) else stack_labels(labels, self.config.tasks, dev)
        w = self._weights(labels, getattr(self, 'train_grouped', None))
        self.model.train()
        if req is not None:      # request-grouped: seq holds one row per request, req the request of each candidate
            probs = self.model.forward_probs_requests(_to_dev(non_seq, dev), _seq_inputs(self.model, seq, dev), req,
                                                      training=True)
        else:
            probs = self.model.forward_probs(_to_dev(non_seq, dev), _seq_inputs(self.model, seq, dev), training=True)
        if next_batch is not None and self.model.sharded:
            self.model.route_ahead(_seq_inputs(self.model, next_batch[1], dev))
        loss = self._loss(y, probs, labels, w)
        self.optimizer.prepare_table_exchange()
        self.optimizer.begin_backward()
        loss.backward()
        self.optimizer.step()
        if self.train_metrics is not None:               # train.py:140-150
            self._update_metrics(self.train_metrics, y, probs.detach(), w)
        if getattr(self, 'train_grouped', None) is not None:
            self.train_grouped.update(self._group_ids(non_seq), y, probs.detach())
        return {'total_loss': loss.detach(), 'probs': probs.detach()}

    @torch.no_grad()
    def val_step(self, batch_data) -> Dict[str, torch.Tensor]:
        """train.py:158-190."""
        non_seq, seq, labels, req = _split_batch(batch_data)
        dev = self.device
        y = labels if isinstance(labels, torch.Tensor) else stack_labels(labels, self.config.tasks, dev)
        w = self._weights(labels, getattr(self, 'val_grouped', None))
        if req is not None:
            probs = self.model.forward_probs_requests(_to_dev(non_seq, dev), _seq_inputs(self.model, seq, dev), req,
                                                      training=False)
        else:
            probs = self.model.forward_probs(_to_dev(non_seq, dev), _seq_inputs(self.model, seq, dev), training=False)
        loss = self._loss(y, probs, labels, w)
        if self.val_metrics is not None:                 # train.py:176-185
            self._update_metrics(self.val_metrics, y, probs, w)
        if getattr(self, 'val_grouped', None) is not None:
            self.val_grouped.update(self._group_ids(non_seq), y, probs)
        return {'total_loss': loss, 'probs': probs}

    def evaluate(self, batches) -> Dict[str, float]:
        """Per task over a list of batches: 'ctr' / 'cvr' (BCE tasks) the exact rank AUC + the Keras
        200-threshold AUC; any other task (trained with MSE, train.py:88-91) mse and mae, as the
        reference reports for regression tasks (train.py:106, evaluate.py:52-54)."""
        weighted = bool(getattr(self.config, 'weighted_loss', False))
        ps, ys, ws = [], [], []
        for b in batches:
            out = self.val_step(b)
            ps.append(out['probs'].cpu().numpy())
            ys.append(stack_labels(b[2], self.config.tasks, 'cpu').numpy())
            if weighted:
                w = stack_weights(b[2], self.config, 'cpu')
                ws.append(np.ones_like(ys[-1]) if w is None else np.clip(np.nan_to_num(w.numpy(), nan=0.0), 0.0,
                                                                       LOSS_WEIGHT_MAX))
        P, Y = np.concatenate(ps, 1), np.concatenate(ys, 1)
        W = np.concatenate(ws, 1).astype(np.float64) if weighted else None
        res = {}
        for i, t in enumerate(self.config.tasks):
            if t in BINARY_TASKS:
                res[f'{t}_auc'] = auc(Y[i], P[i]) if W is None else auc(Y[i], P[i], weights=W[i])
                res[f'{t}_keras_auc'] = keras_auc(Y[i], P[i]) if W is None else keras_auc(Y[i], P[i], weights=W[i])
            elif W is None:
                e = P[i].astype(np.float64) - Y[i].astype(np.float64)
                res[f'{t}_mse'] = float(np.mean(e * e))
                res[f'{t}_mae'] = float(np.mean(np.abs(e)))
            else:                                        # Σ w v / Σ w over the entries with a weight (div_no_nan)
                k = W[i] > 0
                e = P[i][k].astype(np.float64) - Y[i][k].astype(np.float64)
                res[f'{t}_mse'] = float(div_no_nan(np.sum(W[i][k] * e * e), W[i][k].sum()))
                res[f'{t}_mae'] = float(div_no_nan(np.sum(W[i][k] * np.abs(e)), W[i][k].sum()))
        return res

    def train(self, train_batches, val_batches=None, epochs: int = 1) -> Dict:
        """Minimal epoch loop (train.py:192-279): loss history and validation AUC."""
        for ep in range(epochs):
            t0 = time.time()
            losses = [self.train_step(b)['total_loss'] for b in train_batches]
            self.history['train_loss'].append(float(torch.stack(losses).mean()))
            if val_batches:
                self.history['val_metrics'][ep] = self.evaluate(val_batches)
            print(f'epoch {ep + 1}/{epochs} loss {self.history["train_loss"][-1]:.5f} ({time.time() - t0:.1f}s)')
        return self.history

    def fit(self, train_batches, val_batches=None, epochs: int = 10, save_freq: int = 1,
            early_stopping_patience: int = 5, save_optimizer: bool = False) -> Dict:
        """The reference's training loop (train.py:192-279).  Per epoch: the training steps, then the validation
        steps; ``history['train_loss' / 'val_loss']`` get the epoch means (the validation loss is the training
        loss without validation data) and ``history['train_metrics' / 'val_metrics'][epoch]`` the running
        metrics' results; then ``best_model`` on a strict improvement of the validation loss, ``model_epoch_{n}``
        every ``save_freq`` epochs, the early stop after ``early_stopping_patience`` epochs without improvement,
        and the reset of both metric states.  ``final_model`` is saved after the loop.  The per-step losses and
        the metric states stay on the device; each is read once per epoch.  ``save_optimizer``: every checkpoint
        also carries the optimizer state (``save_model(..., include_optimizer=True)``)."""
        if getattr(self, 'train_metrics', None) is None or getattr(self, 'val_metrics', None) is None:
            self.enable_metrics()

        def epoch_mean(losses) -> float:
            # one read of the stacked device scalars; in a data-parallel run the mean over the ranks, so every
            # rank takes the same checkpoint / early-stop decisions
            m = torch.stack(losses).mean()
            if otdist.world() > 1:
                m = m.clone()
                otdist.allreduce_sum_async(m).wait()
                m = m / otdist.world()
            return float(m)

        # (a subclass's one-argument save_model keeps working while the flag is off)
        save = (lambda name: self.save_model(name, include_optimizer=True)) if save_optimizer else self.save_model
        best_val_loss, patience_counter = float('inf'), 0
        for epoch in range(epochs):
            t0 = time.time()
            losses = [self.train_step(b)['total_loss'] for b in train_batches]
            avg_train_loss = epoch_mean(losses)
            if val_batches:
                losses = [self.val_step(b)['total_loss'] for b in val_batches]
                avg_val_loss = epoch_mean(losses)
            else:
                avg_val_loss = avg_train_loss
            self.history['train_loss'].append(avg_train_loss)
            self.history['val_loss'].append(avg_val_loss)
            self.history['train_metrics'][epoch] = self.metric_results(self.train_metrics)
            self.history['val_metrics'][epoch] = self.metric_results(self.val_metrics)
            print(f'epoch {epoch + 1}/{epochs} - train loss {avg_train_loss:.4f}, val loss {avg_val_loss:.4f} '
                  f'({time.time() - t0:.2f}s)')
            if avg_val_loss < best_val_loss:
                best_val_loss, patience_counter = avg_val_loss, 0
                save('best_model')
            else:
                patience_counter += 1
            if (epoch + 1) % save_freq == 0:
                save(f'model_epoch_{epoch + 1}')
            if patience_counter >= early_stopping_patience:
                print(f'early stop at epoch {epoch + 1}')
                break
            self.reset_metrics()
        save('final_model')
        return self.history

    def reset_metrics(self) -> None:
        """Reset every running metric state, the grouped ones included."""
        for m in (self.train_metrics, self.val_metrics, getattr(self, 'train_grouped', None),
                  getattr(self, 'val_grouped', None)):
            if m is not None:
                m.reset_states()

    def progressive_validation(self, batches, period_of=None) -> Dict:
        """The paper's next-batch evaluation ("record the predictions of each mini-batch in evaluation mode, then
        train on that batch"): for every batch ``val_step`` on it, then ``train_step`` on it.  ``period_of(i,
        batch)`` names the batch's period (the paper: the day); at each change of period the validation metrics are
        read (``metric_results``), stored under the period that ended, and reset.  Without ``period_of`` there is
        one period.  The validation states are reset before the first batch, so what they held is not counted.
        Returns ``{'periods': {name: metrics}, 'macro': {metric: mean over the periods}}``."""
        if getattr(self, 'val_metrics', None) is None:
            self.enable_metrics()
        periods: Dict = {}

        def reset() -> None:
            for m in (self.val_metrics, getattr(self, 'val_grouped', None)):
                if m is not None:
                    m.reset_states()

        def close(name) -> None:
            periods[name] = self.metric_results(self.val_metrics)
            reset()

        reset()
        current, seen = None, False
        for i, b in enumerate(batches):
            name = period_of(i, b) if period_of is not None else 0
            if seen and name != current:
                close(current)
            current, seen = name, True
            self.val_step(b)
            self.train_step(b)
        if seen:
            close(current)
        keys = sorted({k for m in periods.values() for k in m})
        macro = {k: float(np.mean([m[k] for m in periods.values() if k in m])) for k in keys}
        return {'periods': periods, 'macro': macro}

    # --------------------------------------------------------------- checkpoint (train.py:281-338)
    def save_model(self, model_name: str, include_optimizer: bool = False) -> None:
        """train.py:281-297: weights, config.json, training_history.json.  ``include_optimizer`` adds
        ``optimizer_state.npz`` (OneTransOptimizer.state_dict: the dense slots, the step count and the tables'
        Adagrad accumulators, per element or per row), so that a run resumed with ``load_model`` continues bit for
        bit; off by default,
        the directory then holds the reference's three files.  Collective with a row-sharded table (every rank
        calls it; rank 0 writes the gathered arrays)."""
        path = self.model_dir / model_name
        path.mkdir(parents=True, exist_ok=True)          # the reference never creates it
        self.model.save_weights(str(path / 'model_weights.npz'))
        with open(path / 'config.json', 'w') as f:
            json.dump(self.config.to_dict(), f, indent=2)
        with open(path / 'training_history.json', 'w') as f:
            # the dense optimizer's step count travels with the history, so a resumed run continues the
            # LR warm-up ramp (apply_warmup) where it stopped
            json.dump(dict(self.history, optimizer_steps=self.optimizer.steps_done), f, indent=2, default=float)
        if include_optimizer:
            state = self.optimizer.state_dict()
            if not (self.model.sharded and self.model._rank() != 0):
                np.savez(path / 'optimizer_state.npz', **state)

    def load_model(self, model_path: str) -> None:
        path = Path(model_path)
        if (path / 'config.json').exists():
            with open(path / 'config.json') as f:
                self.config = OneTransConfig.from_dict(json.load(f))
            self.model = OneTransModel(self.config, device=self.device)
            self.optimizer = OneTransOptimizer(self.model, self.config)
        if (path / 'model_weights.npz').exists():
            self.model.load_weights(str(path / 'model_weights.npz'))
        if (path / 'training_history.json').exists():
            with open(path / 'training_history.json') as f:
                self.history = json.load(f)
            self.optimizer.steps_done = int(self.history.pop('optimizer_steps', 0))
        if (path / 'optimizer_state.npz').exists():      # written by save_model(..., include_optimizer=True)
            with np.load(path / 'optimizer_state.npz', allow_pickle=False) as z:
                self.optimizer.load_state_dict({k: z[k] for k in z.files})


def train_one_trans_model(config_name: str = 'small', batches=None, epochs: int = 10,
                          model_dir: str = './models') -> OneTransTrainer:
    """train.py:341-374 (synthetic batches when none are given)."""
    from .data import make_batch
    config = get_model_config(config_name)
    trainer = OneTransTrainer(config, model_dir)
    if batches is None:
        batches = [make_batch(32, config, seed=1000 + i, seq_lens=[16, 16, 16]) for i in range(4)]
    trainer.train(batches, batches[:1], epochs=epochs)
    return trainer
