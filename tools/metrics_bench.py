"""What the streaming metrics cost at C2 (B 4,096, two tasks), three figures from one process:
  (a) the metric update alone (ot_metrics_update: two launches), HIP events around single calls and around a
      back-to-back run of them;
  (b) train_step with the metrics on against off, in alternating blocks of steps on one trainer;
  (c) the per-step route without them: probs.cpu() + metrics.keras_auc on the host every step (a device-to-host
      copy and a sync per step), in the same alternation.
    python tools/metrics_bench.py [--steps 20] [--rounds 5] [--out FILE.json]
Prints one JSON line (and writes it to --out).  --update-only runs (a) alone on random probabilities without
building the model: the program to put under `rocprofv3 --kernel-trace --stats` for the two kernels' own times
(the event figures of (a) include the host's issue rate)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from recommend_amd import kernels as K
from recommend_amd.config import workload_config
from recommend_amd.metrics import StreamingMetrics, keras_auc
from recommend_amd.model import BINARY_TASKS, OneTransModel
from recommend_amd.trainer import OneTransTrainer

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C2')
ap.add_argument('--steps', type=int, default=20, help='steps per timed block')
ap.add_argument('--rounds', type=int, default=5, help='alternations of the three modes')
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--calls', type=int, default=200, help='(a): timed update calls')
ap.add_argument('--update-only', action='store_true', help='(a) only, on random inputs, no model')
ap.add_argument('--out', default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), 'metrics_bench needs the GPU (no CPU timing stands in for it)'
dev = torch.device('cuda', 0)
cfg = workload_config(args.config)
K.set_matmul_mode(os.environ.get('ONETRANS_MATMUL', 'split'))
cfg.optimizer_config = dict(cfg.optimizer_config, **bench.TRAINABLE_OPT)
B, T = cfg._batch, len(cfg.tasks)
if args.update_only:
    g = torch.Generator(device='cpu').manual_seed(0)
    probs = torch.rand(T, B, generator=g).to(dev)
    labels = (torch.rand(T, B, generator=g) > 0.7).float().to(dev)
    sm = StreamingMetrics(cfg.tasks, dev)
else:
    trainer = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    batches = bench.device_batches(cfg, B, 4, 0, dev)
    trainer.model.inputs_ready = True
    trainer.enable_metrics()
    sm = trainer.train_metrics
    probs = trainer.val_step(batches[0])['probs'].contiguous()
    labels = batches[0][2]


def median(v):
    return float(np.median(v))


# ---- (a) the update alone ------------------------------------------------------------------------------------
for _ in range(20):
    sm.update(labels, probs)
torch.cuda.synchronize()
single = []
for _ in range(args.calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sm.update(labels, probs)
    e1.record()
    single.append((e0, e1))
torch.cuda.synchronize()
single_us = [1e3 * a.elapsed_time(b) for a, b in single]
runs = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        sm.update(labels, probs)
    e1.record()
    torch.cuda.synchronize()
    runs.append(1e3 * e0.elapsed_time(e1) / args.calls)
sm.reset_states()
update = {'update_single_call_us': {'median': median(single_us), 'min': float(np.min(single_us)),
                                    'p90': float(np.percentile(single_us, 90))},
          'update_back_to_back_us': {'median': median(runs), 'min': float(np.min(runs))}}
if args.update_only:
    print(json.dumps(dict({'config': args.config, 'B': B, 'tasks': list(cfg.tasks)}, **update)))
    sys.exit(0)
trainer.val_metrics.reset_states()


# ---- (b), (c) the step, three ways, alternating --------------------------------------------------------------
def block(mode, first):
    """ms per step of one block: device events around it, or the host clock where that is larger."""
    trainer.train_metrics = sm if mode == 'on' else None
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(args.steps):
        b = batches[(first + i) % len(batches)]
        out = trainer.train_step(b, next_batch=batches[(first + i + 1) % len(batches)])
        if mode == 'host':
            p, y = out['probs'].cpu().numpy(), b[2].cpu().numpy()
            for k, t in enumerate(cfg.tasks):
                if t in BINARY_TASKS:
                    keras_auc(y[k], p[k])
    e1.record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    return max(wall, e0.elapsed_time(e1)) / args.steps


for i in range(args.warmup):
    block('on' if i % 2 else 'off', i)
ms = {'off': [], 'on': [], 'host': []}
n = 0
for r in range(args.rounds):
    for mode in ('off', 'on', 'host'):
        ms[mode].append(block(mode, n))
        n += args.steps
trainer.train_metrics = sm

# the host piece alone, after a sync (copy + numpy, no waiting for the step)
torch.cuda.synchronize()
host_only = []
for _ in range(20):
    t0 = time.perf_counter()
    p, y = probs.cpu().numpy(), labels.cpu().numpy()
    for k, t in enumerate(cfg.tasks):
        if t in BINARY_TASKS:
            keras_auc(y[k], p[k])
    host_only.append(1e3 * (time.perf_counter() - t0))

off, on, host = median(ms['off']), median(ms['on']), median(ms['host'])
res = {
    'config': args.config, 'B': B, 'tasks': list(cfg.tasks), 'device': torch.cuda.get_device_name(0),
    'host': os.uname().nodename, 'steps_per_block': args.steps, 'rounds': args.rounds,
    **update,
    'step_ms': {k: {'median': median(v), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in ms.items()},
    'metrics_on_vs_off_pct': 100.0 * (on - off) / off,
    'host_route_vs_off_pct': 100.0 * (host - off) / off,
    'off_spread_pct': 100.0 * (float(np.max(ms['off'])) - float(np.min(ms['off']))) / off,
    'host_copy_plus_keras_auc_ms': median(host_only),
}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
