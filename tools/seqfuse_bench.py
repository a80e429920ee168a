"""Timestamp-aware sequence fusion (seq_fusion='time', ot_seq_time_rows): what the per-call row map costs.

    python3 tools/seqfuse_bench.py [--configs C2,C5] [--rounds 30] [--train C2] [--steps 20]

Per config (its batch and sequence lengths, synthetic times from data.seq_times) two calls are timed in the same
process in interleaved rounds (one call of each per round, HIP events around each call, a synchronise after it):
  (i)  map        ot_seq_time_rows alone on the plan's staged times: the row map, ranks and latest times
  (ii) tokenizer  the tokenizer forward that consumes the map (NS assemble + NS GEMM + sequence projection GEMM)
``--train``: a training step of that config under 'time' and under 'sep' (two models of the same seed, the same
resident batches, alternating steps; only steps whose loss is finite are timed).
Prints one JSON line per measurement.
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--configs', default='C2,C5')
ap.add_argument('--rounds', type=int, default=30)
ap.add_argument('--train', default='C2', help="config of the 'time' vs 'sep' training step ('' = skip)")
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
a = ap.parse_args()

dev = torch.device('cuda')


def to_dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def time_cfg(name):
    from recommend_amd.config import workload_config
    cfg = workload_config(name)
    cfg.seq_fusion = 'time'
    return cfg


def bench_map(name):
    from recommend_amd import kernels as K
    from recommend_amd.data import make_batch
    from recommend_amd.model import OneTransModel, _Tokenize
    cfg = time_cfg(name)
    B = cfg._batch
    model = OneTransModel(cfg, device=dev, seed=0)
    ns, seq, _ = make_batch(B, cfg, seed=11)
    ns_d, seq_d = to_dev(ns), to_dev(seq)
    with torch.no_grad(), K.precision(model.matmul):
        plan = model._plan(ns_d, seq_d)
        nseq = len(plan['time_bufs'])

        def f_map():
            K.seq_time_rows(plan['time_descs'], nseq, B, plan['L_S'], plan['L0'], plan['seq_rows_t'],
                            rank_out=plan['seq_rank'], last_time=plan['last_time'], device=dev)

        def f_tok():
            return _Tokenize.apply(model.flat, model, plan)

        fns = {'map': f_map, 'tokenizer': f_tok}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, fn in fns.items():
                ms[n].append(timed(fn)[0])
    med = {n: float(np.median(v)) for n, v in ms.items()}
    return {'config': name, 'B': B, 'seq_lens': list(cfg._seq_lens), 'L_S': plan['L_S'], 'rounds': a.rounds,
            'map_us': round(1e3 * med['map'], 2), 'tokenizer_us': round(1e3 * med['tokenizer'], 2),
            'map_over_tokenizer': round(med['map'] / med['tokenizer'], 4),
            'min_us': {n: round(1e3 * float(np.min(v)), 2) for n, v in ms.items()}}


def bench_train(name):
    from recommend_amd.data import make_batch
    from recommend_amd.model import OneTransModel
    from recommend_amd.trainer import OneTransTrainer
    tcfg = time_cfg(name)
    scfg = copy.deepcopy(tcfg)
    scfg.seq_fusion = 'sep'
    B = tcfg._batch
    batches = [tuple(to_dev(p) for p in make_batch(B, tcfg, seed=100 + i)) for i in range(4)]   # 'sep' ignores times
    tr = {m: OneTransTrainer(c, model=OneTransModel(c, device=dev, seed=0)) for m, c in (('time', tcfg), ('sep', scfg))}
    ms = {m: [] for m in tr}
    skipped = 0
    for step in range(a.warmup + a.steps):
        for m, t in tr.items():
            dt, out = timed(lambda: t.train_step(batches[step % 4]))
            if step < a.warmup:
                continue
            if bool(torch.isfinite(out['total_loss'])):
                ms[m].append(dt)
            else:
                skipped += 1
    med = {m: float(np.median(v)) for m, v in ms.items()}
    return {'train_step': name, 'B': B, 'steps': a.steps, 'nonfinite_steps_skipped': skipped,
            'time_ms': round(med['time'], 3), 'sep_ms': round(med['sep'], 3),
            'time_over_sep': round(med['time'] / med['sep'], 4),
            'samples_per_s': {m: round(B / (1e-3 * med[m]), 1) for m in med},
            'tokens': {'time': sum(tcfg._seq_lens) + tcfg.num_ns_tokens,
                       'sep': scfg.seq_token_count(scfg._seq_lens) + scfg.num_ns_tokens}}


def main():
    for name in [c for c in a.configs.split(',') if c]:
        print(json.dumps(bench_map(name)), flush=True)
        torch.cuda.empty_cache()
    if a.train:
        print(json.dumps(bench_train(a.train)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
