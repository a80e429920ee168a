"""What config.weighted_loss costs at C2 (B 4,096, two tasks), from one process:
  (a) the new calls alone on random inputs: the weighted loss forward + backward (ot_task_loss_weighted_fwd / _bwd)
      and the weighted metric update (ot_metrics_update_weighted), next to their un-weighted counterparts, HIP events
      around a back-to-back run of each;
  (b) train_step (running metrics enabled) with the switch on against off, in alternating blocks of steps on one
      trainer; the batches carry a sample weight and a click-gated CVR weight as device tensors in both modes (off:
      the keys are inert).  The switch is flipped on the live trainer between blocks: train_step reads
      config.weighted_loss, loss_reduction and task_loss_weights anew in every step, and each mode keeps the running
      metric states that enable_metrics() created under it.
    python tools/weighted_loss_bench.py [--steps 20] [--rounds 5] [--out FILE.json]
Prints one JSON line (and writes it to --out).  --kernels-only runs (a) alone without building the model: the program
to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times (the event figures of (a) include the
host's issue rate)."""
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
from recommend_amd.data import gate_task_weights, make_batch
from recommend_amd.metrics import StreamingMetrics
from recommend_amd.model import OneTransModel
from recommend_amd.trainer import OneTransTrainer

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C2')
ap.add_argument('--steps', type=int, default=20, help='steps per timed block')
ap.add_argument('--rounds', type=int, default=5, help='alternations of the two modes')
ap.add_argument('--warmup', type=int, default=6)
ap.add_argument('--calls', type=int, default=200, help='(a): timed calls per run')
ap.add_argument('--reduction', default='weights')
ap.add_argument('--kernels-only', action='store_true', help='(a) only, on random inputs, no model')
ap.add_argument('--out', default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), 'weighted_loss_bench needs the GPU (no CPU timing stands in for it)'
dev = torch.device('cuda', 0)
cfg = workload_config(args.config)
K.set_matmul_mode(os.environ.get('ONETRANS_MATMUL', 'split'))
cfg.optimizer_config = dict(cfg.optimizer_config, **bench.TRAINABLE_OPT)
B, T = cfg._batch, len(cfg.tasks)


def median(v):
    return float(np.median(v))


# ---- (a) the calls alone ---------------------------------------------------------------------------------------
g = torch.Generator(device='cpu').manual_seed(0)
logits = torch.randn(T, B, generator=g).to(dev)
probs = torch.sigmoid(logits)
labels = (torch.rand(T, B, generator=g) > 0.7).float().to(dev)
weights = (torch.rand(T, B, generator=g) * 3.0 * (torch.rand(T, B, generator=g) > 0.3)).to(dev)
gscale = torch.ones(1, device=dev)
loss, denom, dz = torch.empty(1, device=dev), torch.empty(T, device=dev), torch.empty(T, B, device=dev)
sm_w, sm_u = StreamingMetrics(cfg.tasks, dev, weighted=True), StreamingMetrics(cfg.tasks, dev)


def loss_weighted():
    K.task_loss_weighted_fwd(logits, probs, labels, weights, B, None, T, B, loss, denom, device=dev,
                             reduction=args.reduction)
    K.task_loss_weighted_bwd(probs, labels, weights, B, None, denom, gscale, T, B, dz)


def loss_plain():
    K.task_loss_logits_fwd(logits, probs, labels, T, B, loss, device=dev)
    K.task_loss_logits_bwd(probs, labels, gscale, T, B, dz)


def back_to_back(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(1e3 * e0.elapsed_time(e1) / args.calls)
    return {'median': median(runs), 'min': float(np.min(runs))}


calls = {'loss_fwd_bwd_weighted_us': back_to_back(loss_weighted),
         'loss_fwd_bwd_unweighted_us': back_to_back(loss_plain),
         'metrics_update_weighted_us': back_to_back(lambda: sm_w.update(labels, probs, weights=weights)),
         'metrics_update_unweighted_us': back_to_back(lambda: sm_u.update(labels, probs))}
if args.kernels_only:
    print(json.dumps(dict({'config': args.config, 'B': B, 'tasks': list(cfg.tasks)}, **calls)))
    sys.exit(0)

# ---- (b) the step, switch on against off, alternating ----------------------------------------------------------
trainer = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
batches = []
for i in range(4):
    ns, seq, lab = make_batch(B, cfg, seed=100000 + i)
    lab = gate_task_weights(lab)
    lab['sample_weight'] = np.where(lab['ctr'] > 0.5, 1.0, 4.0).astype(np.float32)
    batches.append(tuple({k: torch.from_numpy(v).to(dev) for k, v in d.items()} for d in (ns, seq, lab)))
trainer.model.inputs_ready = True
states = {}
for mode in ('off', 'on'):
    cfg.weighted_loss = mode == 'on'
    trainer.enable_metrics()
    states[mode] = (trainer.train_metrics, trainer.val_metrics)
cfg.loss_reduction = args.reduction


def block(mode, first):
    """ms per step of one block: device events around it, or the host clock where that is larger."""
    cfg.weighted_loss = mode == 'on'
    trainer.train_metrics, trainer.val_metrics = states[mode]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(args.steps):
        trainer.train_step(batches[(first + i) % len(batches)], next_batch=batches[(first + i + 1) % len(batches)])
    e1.record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    return max(wall, e0.elapsed_time(e1)) / args.steps


for i in range(args.warmup):
    block('on' if i % 2 else 'off', i)
ms = {'off': [], 'on': []}
n = 0
for r in range(args.rounds):
    for mode in ('off', 'on') if r % 2 == 0 else ('on', 'off'):
        ms[mode].append(block(mode, n))
        n += args.steps
off, on = median(ms['off']), median(ms['on'])
res = {
    'config': args.config, 'B': B, 'tasks': list(cfg.tasks), 'reduction': args.reduction,
    'device': torch.cuda.get_device_name(0), 'steps_per_block': args.steps, 'rounds': args.rounds,
    **calls,
    'step_ms': {k: {'median': median(v), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in ms.items()},
    'on_vs_off_pct': 100.0 * (on - off) / off,
    'off_spread_pct': 100.0 * (float(np.max(ms['off'])) - float(np.min(ms['off']))) / off,
}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
