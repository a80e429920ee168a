"""What the user-level AUC costs on the device against the route a user had before it, on the same records:
n = 2^22 records, T = 2 tasks, Zipf-distributed group sizes plus one group of about 5% of the records.
  (a) the ot_grouped_auc call over the filled log (GroupedAUC.result without its D2H copy), HIP events around
      single calls; with --split also the call with no task and with one task, whose differences give the group
      phase and the per-task phase;
  (b) the host route: copy ids, labels and probabilities to the host and run metrics.uauc per task there;
  (c) GroupedAUC.update per 4096-sample step (slice copies into the log), back to back.
    python tools/grouped_auc_bench.py [--n 4194304] [--calls 20] [--out FILE.json]
Prints one JSON line (and writes it to --out).  --call-only runs (a) alone a few times: the program to put under
`rocprofv3 --kernel-trace --stats` for the kernels' own times."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommend_amd import kernels as K
from recommend_amd.metrics import GroupedAUC, uauc

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=1 << 22)
ap.add_argument('--users', type=int, default=1 << 20, help='id range of the Zipf draw')
ap.add_argument('--calls', type=int, default=20, help='timed device calls')
ap.add_argument('--host-runs', type=int, default=3)
ap.add_argument('--batch', type=int, default=4096)
ap.add_argument('--split', action='store_true', help='(a) also with 0 and 1 task computed')
ap.add_argument('--call-only', action='store_true', help='(a) only, 5 calls, no host route')
ap.add_argument('--out', default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), 'grouped_auc_bench needs the GPU (no CPU timing stands in for it)'
dev = torch.device('cuda', 0)
TASKS = ['ctr', 'cvr']
T, n = len(TASKS), args.n

rng = np.random.default_rng(0)
ids = ((rng.zipf(1.2, size=n) - 1) % args.users).astype(np.int64) + 1
ids[rng.permutation(n)[:n // 20]] = 0                      # the crawler: about 5% of the records
ids = ids * 2654435761 % (1 << 40)                         # spread over 40 bits, as hashed user ids are
labels = (rng.random((T, n)) < 0.2).astype(np.float32)
probs = rng.random((T, n), dtype=np.float32)
largest = int(np.bincount(np.unique(ids, return_inverse=True)[1].reshape(-1)).max())
bits = max(1, int(ids.max()).bit_length())

m = GroupedAUC(TASKS, dev, capacity=n, group_bits=bits)
gd, yd, pd = (torch.from_numpy(a).to(dev) for a in (ids, labels, probs))
m.update(gd, yd, pd)
out = torch.empty(T * 4 + 1, dtype=torch.int64, device=dev)


def device_call(mask):
    K.grouped_auc(m._ids, m._probs, m._labels, T, n, m.capacity, bits, mask, out, (out, T * 4), device=dev)


def time_calls(mask, calls):
    for _ in range(3):
        device_call(mask)
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device_call(mask)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


if args.call_only:
    print(json.dumps({'n': n, 'call_ms': stats(time_calls(3, 5))}))
    sys.exit(0)

res = {'n': n, 'tasks': TASKS, 'group_bits': bits, 'distinct_groups': int(len(np.unique(ids))),
       'largest_group': largest, 'device': torch.cuda.get_device_name(0), 'host': os.uname().nodename,
       'workspace_bytes': K.size('ot_grouped_auc_workspace_size', T, n, bits)}
res['device_call_ms'] = stats(time_calls(3, args.calls))
if args.split:
    res['device_call_no_task_ms'] = stats(time_calls(0, args.calls))
    res['device_call_one_task_ms'] = stats(time_calls(1, args.calls))
t0 = time.perf_counter()
dres = m.result()
torch.cuda.synchronize()
res['result_with_copy_ms'] = 1e3 * (time.perf_counter() - t0)

# (b) the host route on the same records: the D2H copies, then metrics.uauc per task
host_ms, copy_ms = [], []
for _ in range(args.host_runs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g, y, p = (t.cpu().numpy() for t in m.state())
    t1 = time.perf_counter()
    hres = [uauc(g, y[i], p[i]) for i in range(T)]
    host_ms.append(1e3 * (time.perf_counter() - t0))
    copy_ms.append(1e3 * (t1 - t0))
res['host_route_ms'] = stats(host_ms)
res['host_copy_ms'] = stats(copy_ms)
res['host_over_device'] = res['host_route_ms']['median'] / res['device_call_ms']['median']
res['results_agree'] = all(abs(dres[f'{t}_uauc'] - hres[i]['uauc']) <= 1e-12 * hres[i]['uauc']
                           and dres[f'{t}_uauc_users'] == hres[i]['users'] for i, t in enumerate(TASKS))
res['uauc'] = {t: dres[f'{t}_uauc'] for t in TASKS}

# (c) the append per step
B = args.batch
steps = n // B
m2 = GroupedAUC(TASKS, dev, capacity=n, group_bits=bits)
per_step = []
for r in range(4):                                         # the first pass is the warm-up
    m2.reset_states()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(steps):
        sl = slice(i * B, (i + 1) * B)
        m2.update(gd[sl], yd[:, sl], pd[:, sl])
    e1.record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    if r:
        per_step.append(1e3 * max(wall, e0.elapsed_time(e1)) / steps)
res['update_per_step_us'] = stats(per_step)
res['update_steps'] = steps

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
