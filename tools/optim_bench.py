"""The dense optimizer step alone: ot_clip_rmsprop against ot_clip_adam on the C2 and T flat layouts (no model:
random weights and gradients in buffers of the layout's size, the layout's own clip segments), in alternating
blocks within one process.  HIP events bracket back-to-back runs of --calls calls after a warm-up; per layout it
reports us per call of each (median and min over the blocks), their ratio and the achieved GB/s at 32 B per
covered element (28 B for the update: read w, g and both slots, write w and both slots; 4 B for the norm pass's
gradient read).
    python tools/optim_bench.py [--layouts C2 T] [--calls 200] [--rounds 7] [--out FILE.json]
--step adds the whole C2 train_step with dense_optimizer 'adam' against 'rmsprop' (bench.py's trainable settings,
one model, the two optimizers swapped between alternating blocks of --steps steps), for information.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommend_amd import kernels as K
from recommend_amd.config import workload_config
from recommend_amd.layout import FlatLayout

ap = argparse.ArgumentParser()
ap.add_argument('--layouts', nargs='+', default=['C2', 'T'])
ap.add_argument('--calls', type=int, default=200, help='calls per timed block')
ap.add_argument('--rounds', type=int, default=7, help='alternations of the two optimizers')
ap.add_argument('--warmup', type=int, default=50)
ap.add_argument('--step', action='store_true', help='also time the whole C2 train_step under both optimizers')
ap.add_argument('--steps', type=int, default=20, help='--step: steps per timed block')
ap.add_argument('--out', default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), 'optim_bench needs the GPU (no CPU timing stands in for it)'
dev = torch.device('cuda', 0)


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def layout_times(name):
    cfg = workload_config(name)
    L = FlatLayout(cfg, cfg.ns_input_width())
    gen = torch.Generator(device='cpu').manual_seed(0)
    w = (0.05 * torch.randn(L.total, generator=gen)).to(dev)
    g = (0.01 * torch.randn(L.total, generator=gen)).to(dev)
    slots = {k: (torch.zeros_like(w), torch.zeros_like(w)) for k in ('rmsprop', 'adam')}
    segs = torch.from_numpy(L.segments.reshape(-1)).to(dev)
    nseg, mx = L.segments.shape[0], L.max_seg_elems
    covered = int((L.segments[:, 1] * L.segments[:, 2]).sum())
    step = [0]

    def call(kind):
        a, b = slots[kind]
        if kind == 'rmsprop':
            K.clip_rmsprop(w, g, a, b, segs, nseg, mx, 1e-5, 0.9, 1e-7, 0.9, 90.0, device=dev)
        else:
            step[0] += 1
            K.clip_adam(w, g, a, b, segs, nseg, mx, 1e-5, 0.9, 0.999, 1e-8, step[0], 90.0, device=dev)

    def block(kind):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.calls):
            call(kind)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.calls

    for kind in ('rmsprop', 'adam'):
        for _ in range(args.warmup):
            call(kind)
    us = {'rmsprop': [], 'adam': []}
    for _ in range(args.rounds):
        for kind in ('rmsprop', 'adam'):
            us[kind].append(block(kind))
    assert bool(torch.isfinite(w).all())
    r, a = float(np.median(us['rmsprop'])), float(np.median(us['adam']))
    return {'segments': int(nseg), 'covered_elems': covered, 'flat_elems': int(L.total),
            'vector_segments': int(((L.segments[:, [0, 2, 3]] % 4) == 0).all(1).sum()),
            'rmsprop_us': stats(us['rmsprop']), 'adam_us': stats(us['adam']), 'adam_over_rmsprop': a / r,
            'rmsprop_gbs': 32.0 * covered / (r * 1e-6) / 1e9, 'adam_gbs': 32.0 * covered / (a * 1e-6) / 1e9}


def step_times():
    import bench
    from recommend_amd.model import OneTransModel
    from recommend_amd.trainer import OneTransOptimizer, OneTransTrainer
    K.set_matmul_mode(os.environ.get('ONETRANS_MATMUL', 'split'))
    cfg = workload_config('C2')
    cfg.optimizer_config = dict(cfg.optimizer_config, **bench.TRAINABLE_OPT)
    trainer = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    acfg = workload_config('C2')
    acfg.optimizer_config = dict(cfg.optimizer_config, dense_optimizer='adam', beta1=0.9, beta2=0.999)
    opts = {'rmsprop': trainer.optimizer, 'adam': OneTransOptimizer(trainer.model, acfg)}
    assert opts['adam'].kind == 'adam' and opts['rmsprop'].kind == 'rmsprop'
    batches = bench.device_batches(cfg, cfg._batch, 4, 0, dev)
    trainer.model.inputs_ready = True

    def block(kind, first):
        trainer.optimizer = opts[kind]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(args.steps):
            out = trainer.train_step(batches[(first + i) % 4], next_batch=batches[(first + i + 1) % 4])
        e1.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out['total_loss']))
        return max(1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)) / args.steps

    n = 0
    for i in range(4):
        block('adam' if i % 2 else 'rmsprop', n)
        n += args.steps
    ms = {'rmsprop': [], 'adam': []}
    for _ in range(args.rounds):
        for kind in ('rmsprop', 'adam'):
            ms[kind].append(block(kind, n))
            n += args.steps
    r, a = float(np.median(ms['rmsprop'])), float(np.median(ms['adam']))
    return {'config': 'C2', 'B': cfg._batch, 'steps_per_block': args.steps, 'rmsprop_ms': stats(ms['rmsprop']),
            'adam_ms': stats(ms['adam']), 'adam_vs_rmsprop_pct': 100.0 * (a - r) / r}


res = {'device': torch.cuda.get_device_name(0), 'calls_per_block': args.calls, 'rounds': args.rounds,
       'layouts': {name: layout_times(name) for name in args.layouts}}
if args.step:
    res['train_step'] = step_times()
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
