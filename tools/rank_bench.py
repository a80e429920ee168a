"""Per-request top-K ranking on the device (OneTransServer.rank, ot_rank_topk) against the path it replaces.

    python3 tools/rank_bench.py [--config C2] [--shapes 64x512,1x512] [--k 32] [--rounds 30]
    python3 tools/rank_bench.py --extreme        # correctness only: one request with 2^20 candidates

Per shape RxN (R requests with N candidates each) three calls are timed in the same process, in interleaved
rounds (one call of each per round, HIP events around each call, a synchronise after it), stage I cached:
  (i)   score        stage II alone: {task: probs} left on the device
  (ii)  rank         stage II + ot_rank_topk: index / score / count left on the device
  (iii) score+host   stage II, one copy of all T*C probabilities to the host, numpy fused score, per-request
                     argpartition and sort of the k winners
Prints one JSON line per shape: the three medians (ms), (ii)/(i), (ii)/(iii), and whether the device ranking and
the host one agree.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C2')
ap.add_argument('--shapes', default='64x512,1x512', help='RxN: R requests with N candidates each')
ap.add_argument('--k', type=int, default=32)
ap.add_argument('--rounds', type=int, default=30)
ap.add_argument('--extreme', action='store_true', help='one request with 2^20 candidates, checked against numpy')
a = ap.parse_args()

dev = torch.device('cuda')


def extreme():
    """ot_rank_topk alone on one request of 2^20 candidates, scores drawn from 2^16 values (long tie runs, the
    k-th boundary inside one), K = 1024, against a numpy sort by (score descending, index ascending)."""
    from recommend_amd import kernels as K
    C, Kk = 1 << 20, 1024
    rng = np.random.default_rng(0)
    p = (rng.integers(0, 1 << 16, C).astype(np.float32) / np.float32(1 << 16))
    p[rng.integers(0, C, 64)] = np.nan
    probs = torch.from_numpy(p).to(dev).view(1, C)
    req = torch.zeros(C, dtype=torch.int32, device=dev)
    idx = torch.empty(1, Kk, dtype=torch.int32, device=dev)
    sc = torch.empty(1, Kk, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    K.rank_topk(probs, C, 1, [1.0], 'sum', req, C, 1, Kk, idx, sc, cnt, device=dev)
    e1.record()
    torch.cuda.synchronize()
    key = np.where(np.isnan(p), -np.inf, p.astype(np.float64))               # no -inf among the scores: NaN last
    ref = np.lexsort((np.arange(C), -key))[:Kk]
    ok = bool((idx.cpu().numpy()[0] == ref).all() and int(cnt[0]) == Kk
              and (sc.cpu().numpy()[0] == p[ref]).all())
    print(json.dumps({'extreme': {'R': 1, 'C': C, 'K': Kk, 'first_call_ms': round(e0.elapsed_time(e1), 3),
                                  'matches_numpy': ok}}))
    return 0 if ok else 1


def bench_shape(srv, cfg, Rq, N):
    from recommend_amd.data import make_batch
    C, k = Rq * N, min(a.k, N)
    _, seq_r, _ = make_batch(Rq, cfg, seed=11)
    ns_c, _, _ = make_batch(C, cfg, seed=12)
    req = np.repeat(np.arange(Rq), N)
    to = lambda d: {k_: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k_, v in d.items()}
    seq_r_d, ns_c_d = to(seq_r), to(ns_c)
    req_h = torch.from_numpy(req.astype(np.int32))          # host indices: validated without a read-back
    tasks = list(cfg.tasks)
    cache = srv.encode_requests(seq_r_d)

    def f_score():
        return srv.score(cache, req_h, ns_c_d)

    def f_rank():
        return srv.rank(cache, req_h, ns_c_d, k)

    def f_host():
        out = srv.score(cache, req_h, ns_c_d)
        p = torch.stack([out[t][:, 0] for t in tasks]).cpu().numpy()         # one copy of all T*C
        f = p.sum(0, dtype=np.float32).reshape(Rq, N)
        if k < N:
            top = np.argpartition(-f, k - 1, axis=1)[:, :k]
        else:
            top = np.broadcast_to(np.arange(N), (Rq, N)).copy()
        order = np.argsort(-np.take_along_axis(f, top, 1), axis=1, kind='stable')
        top = np.take_along_axis(top, order, 1)
        return top + (np.arange(Rq) * N)[:, None], np.take_along_axis(f, top, 1)

    fns = {'score': f_score, 'rank': f_rank, 'score_host': f_host}
    with torch.no_grad():
        for fn in fns.values():                               # warm every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[n].append(e0.elapsed_time(e1))
        got = f_rank()
        host_idx, host_f = f_host()
    med = {n: float(np.median(v)) for n, v in ms.items()}
    # ties aside (the host path breaks them differently), the two rankings hold the same scores in the same order
    same_scores = bool(np.allclose(got['score'].cpu().numpy(), host_f, rtol=0, atol=1e-6))
    same_index = float((got['index'].cpu().numpy() == host_idx).mean())
    return {'config': a.config, 'R': Rq, 'C': C, 'k': k, 'rounds': a.rounds,
            'score_ms': round(med['score'], 4), 'rank_ms': round(med['rank'], 4),
            'score_host_ms': round(med['score_host'], 4),
            'rank_over_score': round(med['rank'] / med['score'], 4),
            'rank_over_score_host': round(med['rank'] / med['score_host'], 4),
            'min_ms': {n: round(float(np.min(v)), 4) for n, v in ms.items()},
            'scores_agree': same_scores, 'index_agreement': round(same_index, 4)}


def main():
    if a.extreme:
        return extreme()
    from recommend_amd.config import workload_config
    from recommend_amd.model import OneTransModel
    from recommend_amd.serving import OneTransServer
    cfg = workload_config(a.config)
    srv = OneTransServer(OneTransModel(cfg, device=dev, seed=0))
    for shape in a.shapes.split(','):
        Rq, N = (int(v) for v in shape.lower().split('x'))
        print(json.dumps(bench_shape(srv, cfg, Rq, N)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
