"""The embedding-table optimizers (optimizer_config['sparse_optimizer']): element-wise Adagrad ('adagrad',
ot_sparse_adagrad) against row-wise Adagrad ('rowwise_adagrad', ot_sparse_adagrad_rowwise) at C2's shape.

    python3 tools/sparse_optim_bench.py [--rounds 20] [--steps 20] [--warmup 5] [--out FILE.json]

Update: one C2 train_step's own (key, gradient row) pairs per table (copied just before optimizer.step()), then per
table the one-call update of either kind on those pairs, and the dense form (ot_sparse_grad_dense's buffer, then
ot_dense_adagrad / ot_dense_adagrad_rowwise: what a data-parallel run applies to a densely exchanged table) on every
table under 512 MB; ``apply_*``: the apply kernels alone (ot_sparse_finish / ot_sparse_finish_rowwise on one
prepared workspace: the clip scale's one-thread kernel and the apply kernel).  HIP events around each call, a synchronise after it, medians over ``--rounds`` rounds that
alternate the kinds.  ``apply_bytes``: the table and accumulator traffic of the touched rows, 4E floats per row
(weight and accumulator, each read and written) against 2E + 2; both also read the row's gradient sum (E).
Step: C2 train_step with either kind, two trainers of one seed on the same resident batches, alternating steps;
steps with a non-finite loss are not counted.
State: OneTransOptimizer.state_nbytes() of both.
Prints one JSON line per measurement; ``--out`` also writes them as one JSON list.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=20)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda')
KINDS = ('adagrad', 'rowwise_adagrad')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def to_dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def trainers():
    from recommend_amd.config import workload_config
    from recommend_amd.model import OneTransModel
    from recommend_amd.trainer import OneTransTrainer
    out = {}
    for kind in KINDS:
        cfg = workload_config('C2')
        cfg.optimizer_config = dict(cfg.optimizer_config, sparse_optimizer=kind)
        out[kind] = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    return out


def capture_pairs(tr, batch):
    """One train_step; the (table, keys, gradient rows) it queued, joined per table, copied before the update."""
    opt, got = tr.optimizer, []
    real = opt.step

    def step():
        got.extend((n, k.reshape(-1).clone(), g.reshape(-1, g.shape[-1]).clone())
                   for (n, k, g) in opt._join_pending(tr.model._pending_sparse))
        real()

    opt.step = step
    try:
        tr.train_step(batch)
    finally:
        del opt.step
    torch.cuda.synchronize()
    return got


def median_us(fns):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(a.rounds):                            # the order turns round every round (A B, B A, ...)
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            ms[k].append(timed(fns[k])[0])
    return ({k: round(1e3 * float(np.median(v)), 2) for k, v in ms.items()},
            {k: round(1e3 * float(np.min(v)), 2) for k, v in ms.items()})


def bench_update(name, table, keys, grads):
    from recommend_amd import kernels as K
    rows, E = table.shape
    n = keys.numel()
    w = table.clone()                                    # the trainers' tables stay as they are
    acc_el = torch.full_like(w, 0.1)
    acc_rw = torch.full((rows,), 0.1, device=dev)
    uniq = int(torch.unique(keys[(keys >= 0) & (keys < rows)]).numel())
    fns = {
        'adagrad': lambda: K.sparse_adagrad(w, acc_el, E, rows, keys, grads, n, 0.1, 1e-7, 120.0, device=dev),
        'rowwise_adagrad': lambda: K.sparse_adagrad_rowwise(w, acc_rw, E, rows, keys, grads, n, 0.1, 1e-7, 120.0,
                                                            device=dev),
    }
    # the apply kernels alone: the second phase of the two-phase form on one prepared workspace
    ws = K.sparse_workspace(n, E, dev)
    sumsq = torch.zeros(1, device=dev)
    K.sparse_prepare(E, rows, keys, grads, n, sumsq, ws)
    fns['apply_adagrad'] = lambda: K.sparse_finish(w, acc_el, E, n, 0.1, 1e-7, 120.0, sumsq, ws)
    fns['apply_rowwise_adagrad'] = lambda: K.sparse_finish_rowwise(w, acc_rw, E, n, 0.1, 1e-7, 120.0, sumsq, ws)
    dense = rows * E * 4 <= 512 * 2 ** 20
    if dense:
        g = torch.zeros(rows, E, device=dev)
        K.sparse_grad_dense(E, rows, keys, grads, n, g, device=dev)
        fns['dense_adagrad'] = lambda: K.dense_adagrad(w, acc_el, g, rows, E, 0.1, 1e-7, 120.0, device=dev)
        fns['dense_rowwise_adagrad'] = lambda: K.dense_adagrad_rowwise(w, acc_rw, g, rows, E, 0.1, 1e-7, 120.0,
                                                                       device=dev)
    med, mn = median_us(fns)
    res = {'update': name, 'rows': rows, 'E': E, 'pairs': n, 'unique_rows': uniq, 'rounds': a.rounds, 'us': med,
           'min_us': mn, 'rowwise_over_adagrad': round(med['rowwise_adagrad'] / med['adagrad'], 4),
           'apply_rowwise_over_adagrad': round(med['apply_rowwise_adagrad'] / med['apply_adagrad'], 4),
           'apply_bytes': {'adagrad': uniq * 4 * E * 4, 'rowwise_adagrad': uniq * (2 * E + 2) * 4}}
    if dense:
        res['dense_rowwise_over_adagrad'] = round(med['dense_rowwise_adagrad'] / med['dense_adagrad'], 4)
    return res


def bench_step(tr, batches):
    ms = {k: [] for k in tr}
    bad = {k: 0 for k in tr}
    for step in range(a.warmup + a.steps):
        for k in (list(tr) if step % 2 == 0 else list(tr)[::-1]):
            t = tr[k]
            dt, out = timed(lambda: t.train_step(batches[step % len(batches)]))
            if step < a.warmup:
                continue
            if bool(torch.isfinite(out['total_loss'])):
                ms[k].append(dt)
            else:
                bad[k] += 1
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {'train_step': 'C2', 'B': batches[0][2]['ctr'].shape[0], 'steps': a.steps, 'non_finite_steps': bad,
            'ms': {k: round(v, 3) for k, v in med.items()},
            'rowwise_over_adagrad': round(med['rowwise_adagrad'] / med['adagrad'], 4),
            'spread_ms': {k: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in ms.items()}}


def main():
    from recommend_amd.data import make_batch
    res = []

    def emit(r):
        res.append(r)
        print(json.dumps(r), flush=True)

    tr = trainers()
    cfg = tr['adagrad'].config
    batches = [tuple(to_dev(p) for p in make_batch(cfg._batch, cfg, seed=100 + i)) for i in range(4)]
    nb = {k: t.optimizer.state_nbytes() for k, t in tr.items()}
    tables = {n: list(t.shape) for n, t in tr['adagrad'].model.tables.items()}
    emit({'state_nbytes': nb, 'tables': tables, 'saved_bytes': nb['adagrad'] - nb['rowwise_adagrad'],
          'table_bytes': sum(r * e * 4 for r, e in tables.values()),
          'rowwise_over_adagrad': round(nb['rowwise_adagrad'] / nb['adagrad'], 4)})
    pairs = capture_pairs(tr['adagrad'], batches[0])
    tr['rowwise_adagrad'].train_step(batches[0])         # (both trainers one step in)
    for name, keys, grads in pairs:
        emit(bench_update(name, tr['adagrad'].model.tables[name], keys, grads))
        torch.cuda.empty_cache()
    del pairs
    emit(bench_step(tr, batches))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
