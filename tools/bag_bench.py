"""Multi-valued NS features (bag_features; ot_ns_bag_pool / ot_ns_bag_grad_pack): what the bags cost at C2's batch.

    python3 tools/bag_bench.py [--rounds 20] [--train-cap 32] [--steps 20] [--out FILE.json]

Kernels: B = 4096 samples, 4 bags per call over one 1,000,000-row table, E = 16 and E = 64, cap 4 / 32 / 128, bag
lengths binomial with mean cap / 4, Zipf(1.1) ids (data.bag_ids).  Timed per shape, HIP events around each call, a
synchronise after it, medians over ``--rounds`` interleaved rounds:
  pool      ot_ns_bag_pool; its algorithmic bytes (valid rows read once, ids, coefficients and pooled rows written)
            over its time, against the device copy rate measured here on tools/hbm_calib.py's 1 GiB copy
  pack      ot_ns_bag_grad_pack
  adagrad   ot_sparse_adagrad on the pack's B * cap * 4 (key, row) pairs, and on the valid pairs alone (compacted on
            the host side of the benchmark): the difference is what the padded layout's empty slots cost the sort
``--train-cap``: a whole train_step of C2 with 4 bag features (two over emb.ns, two over emb.seq_item, that cap)
against C2 without them: two models of one seed, resident batches, alternating steps.
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
ap.add_argument('--train-cap', type=int, default=32, help='cap of the train_step comparison (0 = skip)')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda')
B, NBAGS, ROWS = 4096, 4, 1_000_000


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def to_dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def copy_rate():
    """tools/hbm_calib.py's copy (1 GiB read + 1 GiB written), timed: bytes/s of HBM traffic."""
    n = (1 << 30) // 4
    x = torch.empty(n, device=dev).uniform_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    ms = [timed(lambda: y.copy_(x))[0] for _ in range(10)]
    return 2.0 * n * 4 / (1e-3 * float(np.median(ms)))


def bench_kernels(E, cap, hbm):
    from recommend_amd import kernels as K
    from recommend_amd.data import bag_ids
    table = torch.empty(ROWS, E, device=dev).uniform_(-0.05, 0.05)
    accum = torch.full_like(table, 0.1)
    ids_h = [bag_ids(17 * cap + E + f, B, ROWS, cap, cap / 4.0) for f in range(NBAGS)]
    ids = [torch.from_numpy(i).to(dev) for i in ids_h]
    ld = NBAGS * E
    descs = K.ns_bag_descs([dict(table=table, ids=ids[f], weights=None, row_offset=0, num_rows=ROWS, ids_stride=cap,
                                 width=E, cap=cap, col=f * E, pooling='mean') for f in range(NBAGS)])
    n = NBAGS * B * cap
    valid = int(sum((i >= 0).sum() for i in ids_h))
    out = torch.zeros(B, ld, device=dev)
    coef = torch.zeros(n, device=dev)
    dmat = torch.empty(B, ld, device=dev).normal_()
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    grads = torch.empty(n, E, device=dev)
    K.ns_bag_pool(descs, NBAGS, B, out, ld, coef)
    K.ns_bag_grad_pack(descs, NBAGS, B, dmat, ld, coef, keys, grads)
    sel = torch.nonzero(keys >= 0).reshape(-1)
    keys_v, grads_v = keys[sel].contiguous(), grads[sel].contiguous()
    fns = {
        'pool': lambda: K.ns_bag_pool(descs, NBAGS, B, out, ld, coef),
        'pack': lambda: K.ns_bag_grad_pack(descs, NBAGS, B, dmat, ld, coef, keys, grads),
        'adagrad_padded': lambda: K.sparse_adagrad(table, accum, E, ROWS, keys, grads, n, 0.1, 1e-7, 120.0, device=dev),
        'adagrad_valid': lambda: K.sparse_adagrad(table, accum, E, ROWS, keys_v, grads_v, keys_v.numel(), 0.1, 1e-7,
                                                  120.0, device=dev),
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    uniq = int(torch.unique(keys_v).numel())
    pool_bytes = valid * E * 4 + n * 8 + n * 4 + B * ld * 4
    rate = pool_bytes / (1e-3 * med['pool'])
    return {'E': E, 'cap': cap, 'B': B, 'bags': NBAGS, 'slots': n, 'valid_slots': valid, 'unique_rows': uniq,
            'rounds': a.rounds, 'us': {k: round(1e3 * v, 2) for k, v in med.items()},
            'min_us': {k: round(1e3 * float(np.min(v)), 2) for k, v in ms.items()},
            'pool_bytes': pool_bytes, 'pool_GBps': round(rate / 1e9, 1), 'pool_over_copy_rate': round(rate / hbm, 4),
            'pool_unique_row_bytes': uniq * E * 4,
            'padded_sort_cost_us': round(1e3 * (med['adagrad_padded'] - med['adagrad_valid']), 2)}


def bench_train(cap):
    import copy
    from recommend_amd.config import workload_config
    from recommend_amd.data import make_batch
    from recommend_amd.model import OneTransModel
    from recommend_amd.trainer import OneTransTrainer
    plain = workload_config('C2')
    bag = copy.deepcopy(plain)
    fc = bag.feature_config
    fc['user_features'] = fc['user_features'] + ['tags_a', 'tags_b']
    fc['item_features'] = fc['item_features'] + ['sim_a', 'sim_b']
    bag.bag_features = {'tags_a': {'cardinality': 100_000, 'pooling': 'mean'},
                        'tags_b': {'cardinality': 100_000, 'pooling': 'sum'},
                        'sim_a': {'table': 'seq_item', 'pooling': 'mean'},
                        'sim_b': {'table': 'seq_item', 'pooling': 'mean'}}
    Bt = plain._batch
    from recommend_amd.data import criteo_batch
    caps = {n: (cap, cap / 4.0) for n in bag.bag_features}
    batches = {'bags': [tuple(to_dev(p) for p in criteo_batch(Bt, bag, seed=100 + i, bags=caps)) for i in range(4)],
               'plain': [tuple(to_dev(p) for p in make_batch(Bt, plain, seed=100 + i)) for i in range(4)]}
    tr = {m: OneTransTrainer(c, model=OneTransModel(c, device=dev, seed=0))
          for m, c in (('bags', bag), ('plain', plain))}
    ms = {m: [] for m in tr}
    for step in range(a.warmup + a.steps):
        for m, t in tr.items():
            dt, out = timed(lambda: t.train_step(batches[m][step % 4]))
            if step >= a.warmup and bool(torch.isfinite(out['total_loss'])):
                ms[m].append(dt)
    med = {m: float(np.median(v)) for m, v in ms.items()}
    return {'train_step': 'C2', 'B': Bt, 'cap': cap, 'bag_features': 4, 'steps': a.steps,
            'bags_ms': round(med['bags'], 3), 'plain_ms': round(med['plain'], 3),
            'bags_over_plain': round(med['bags'] / med['plain'], 4),
            'spread_ms': {m: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for m, v in ms.items()}}


def main():
    res = []
    hbm = copy_rate()
    res.append({'copy_rate_GBps': round(hbm / 1e9, 1), 'what': '1 GiB device copy, read + write bytes over time'})
    print(json.dumps(res[-1]), flush=True)
    for E in (16, 64):
        for cap in (4, 32, 128):
            res.append(bench_kernels(E, cap, hbm))
            print(json.dumps(res[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.train_cap:
        res.append(bench_train(a.train_cap))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
