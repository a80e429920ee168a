"""Request-grouped training against the per-sample step at C2 (C = 4,096 candidates, c candidates per request):
  (a) train_step on the request-grouped 4-tuple against train_step on data.expand_requests of the same batch
      (the existing path), one trainer, one process, the two arms alternating in blocks, warmed up, device
      events around every step, the median over >= 20 steps per arm; the expanded arm's spread over its blocks;
  (b) the two cached-attention kernels alone (ot_attn_fwd_cached_lse, ot_attn_bwd_cached) at C2's first-layer
      (Kq = n) and last-layer (Kq = 1) shapes.
    python tools/request_train_bench.py [--cands 1,2,4,8,16] [--steps 5] [--rounds 5] [--out FILE.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from recommend_amd import kernels as K
from recommend_amd.config import workload_config
from recommend_amd.data import expand_requests, make_request_batch
from recommend_amd.model import OneTransModel
from recommend_amd.span_block import request_schedule
from recommend_amd.trainer import OneTransTrainer, stack_labels

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C2')
ap.add_argument('--candidates', type=int, default=4096, help='C, candidates per batch')
ap.add_argument('--cands', default='1,2,4,8,16', help='candidates per request, comma separated')
ap.add_argument('--steps', type=int, default=5, help='steps per block')
ap.add_argument('--rounds', type=int, default=5, help='alternations of the two arms (steps * rounds >= 20)')
ap.add_argument('--warmup', type=int, default=4, help='warm-up steps per arm and c')
ap.add_argument('--calls', type=int, default=50, help='(b): timed calls per kernel and shape')
ap.add_argument('--out', default=None)
args = ap.parse_args()
assert args.steps * args.rounds >= 20, 'at least 20 timed steps per arm'

assert torch.cuda.is_available(), 'request_train_bench needs the GPU (no CPU timing stands in for it)'
dev = torch.device('cuda', 0)
cfg = workload_config(args.config)
K.set_matmul_mode(os.environ.get('ONETRANS_MATMUL', 'split'))
cfg.optimizer_config = dict(cfg.optimizer_config, **bench.TRAINABLE_OPT)
C = args.candidates
trainer = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
trainer.model.inputs_ready = True


def resident(batch):
    """The batch on the device (labels stacked), as bench.device_batches keeps them."""
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    out = (t(batch[0]), t(batch[1]), stack_labels(batch[2], cfg.tasks, dev))
    return out + (torch.from_numpy(batch[3]).to(dev),) if len(batch) == 4 else out


def median(v):
    return float(np.median(v))


def timed_steps(batch, n):
    evs = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        trainer.train_step(batch)
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


# ---- (a) the step, two ways, alternating ---------------------------------------------------------------------
steps = {}
for c in [int(x) for x in args.cands.split(',')]:
    R = C // c
    host = make_request_batch(R, c, cfg, seed=100000 + c)
    arms = {'grouped': resident(host), 'expanded': resident(expand_requests(host))}
    for name, b in arms.items():
        timed_steps(b, args.warmup)
    ms = {'grouped': [], 'expanded': []}
    blocks = {'grouped': [], 'expanded': []}
    for r in range(args.rounds):
        for name in (('grouped', 'expanded') if r % 2 == 0 else ('expanded', 'grouped')):
            t = timed_steps(arms[name], args.steps)
            ms[name] += t
            blocks[name].append(median(t))
    g, e = median(ms['grouped']), median(ms['expanded'])
    steps[str(c)] = {
        'R': R, 'grouped_ms': g, 'expanded_ms': e, 'grouped_over_expanded': g / e,
        'grouped_min_ms': float(np.min(ms['grouped'])), 'expanded_min_ms': float(np.min(ms['expanded'])),
        'expanded_block_spread_pct': 100.0 * (max(blocks['expanded']) - min(blocks['expanded'])) / e,
        'grouped_block_spread_pct': 100.0 * (max(blocks['grouped']) - min(blocks['grouped'])) / g,
        'timed_steps_per_arm': len(ms['grouped']),
    }
    print(f'c={c}: grouped {g:.3f} ms, expanded {e:.3f} ms', file=sys.stderr, flush=True)
    del arms
    torch.cuda.empty_cache()

# ---- (b) the two kernels alone -------------------------------------------------------------------------------
d, H = cfg.hidden_dim, cfg.num_heads
hd = d // H
L_S = sum(cfg._seq_lens) + len(cfg._seq_lens) - 1
sched = request_schedule(cfg, L_S)
kernels = {}
gen = torch.Generator(device='cpu').manual_seed(0)
for label, e in (('first_layer', sched[0]), ('last_layer', sched[-1])):
    Ic, n, Kq = e['s'], e['n'], e['kN']
    for c in (1, 8):
        R = C // c
        qkv = torch.randn(C * n, 3 * d, generator=gen).to(dev)
        kv = torch.randn(R * Ic, 3 * d, generator=gen).to(dev)
        dout = torch.randn(C * Kq, d, generator=gen).to(dev)
        req = torch.arange(C, dtype=torch.int32, device=dev) // c
        req_start = torch.arange(R + 1, dtype=torch.int32, device=dev) * c
        out, lse = torch.empty(C * Kq, d, device=dev), torch.empty(C * H * Kq, device=dev)
        dqkv, dkv = torch.zeros(C * n, 3 * d, device=dev), torch.zeros(R * Ic, 3 * d, device=dev)
        fwd = lambda: K.attn_fwd_cached(qkv, 3 * d, (kv, d), 3 * d, req, C, H, Ic, n, Kq, hd, out, lse)
        bwd = lambda: K.attn_bwd_cached(qkv, 3 * d, (kv, d), 3 * d, req_start, R, C, H, Ic, n, Kq, hd, out, dout, lse,
                                        dqkv, (dkv, d))
        for name, fn in (('fwd_cached_lse', fwd), ('bwd_cached', bwd)):
            for _ in range(5):
                fn()
            evs = []
            for _ in range(args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            us = [1e3 * a.elapsed_time(b) for a, b in evs]
            kernels[f'{label}_c{c}_{name}'] = {'Ic': Ic, 'n': n, 'Kq': Kq, 'C': C, 'R': R, 'median_us': median(us),
                                               'min_us': float(np.min(us))}

res = {'config': args.config, 'C': C, 'device': torch.cuda.get_device_name(0), 'matmul': K.matmul_mode(),
       'steps_per_block': args.steps, 'rounds': args.rounds, 'step': steps, 'kernels': kernels}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
