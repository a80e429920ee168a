"""Serving throughput: two-stage cached inference (recommend_amd/serving.py) vs one full forward per
(request, candidate) sample (the reference engine's batch_inference, examples/inference_example.py:131).

    python3 tools/serve_bench.py [--config C2] [--requests 64] [--cands 64] [--iters 20] [--cache-dtype fp32|bf16|both]

Prints one JSON line: candidates/s of both paths (HIP-event timed, inputs resident on the GPU), the
stage-I / stage-II split, and the max |prob| difference between the two paths.

--cache-dtype bf16 / both adds 'cache_dtypes': per request-cache precision (OneTransServer(cache_dtype=)) the
stage-I ms (with the bf16 pack), stage-II ms, the cache's bytes, max |prob| difference against the full forward and
the exact AUC against the batch's teacher labels; with 'both' the two servers alternate inside one process, --rounds
times, and the medians and the min..max spread are reported.  'extend_ms': dL = 4 events appended to the encoded
cache, with reserve (bf16: in place) and without (bf16: one reallocation; fp32: torch.cat of every layer) — on the
configuration without its pyramid when that prunes before the last layer (extend_requests refuses it then).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommend_amd.config import workload_config
from recommend_amd.data import make_batch
from recommend_amd.metrics import auc
from recommend_amd.model import OneTransModel
from recommend_amd.serving import OneTransServer

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C2')
ap.add_argument('--requests', type=int, default=64)
ap.add_argument('--cands', type=int, default=64, help='candidates per request')
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--cache-dtype', choices=['fp32', 'bf16', 'both'], default='fp32')
ap.add_argument('--rounds', type=int, default=5, help='alternated measurement rounds per cache dtype')
a = ap.parse_args()

dev = torch.device('cuda')
cfg = workload_config(a.config)
model = OneTransModel(cfg, device=dev, seed=0)
Rq, C = a.requests, a.requests * a.cands
ns_r, seq_r, _ = make_batch(Rq, cfg, seed=11)
ns_c, _, lab_c = make_batch(C, cfg, seed=12)
req = np.repeat(np.arange(Rq), a.cands)
to = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
seq_r_d, ns_c_d = to(seq_r), to(ns_c)
seq_full_d = to({k: v[req] for k, v in seq_r.items()})
req_d = torch.from_numpy(req.astype(np.int32)).to(dev)
srv = OneTransServer(model)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters, out


with torch.no_grad():
    t_full, p_full = timed(lambda: model((ns_c_d, seq_full_d), training=False))
    t_cached, p_cached = timed(lambda: srv.score(srv.encode_requests(seq_r_d), req_d, ns_c_d))
    t_s1, cache = timed(lambda: srv.encode_requests(seq_r_d))
    t_s2, _ = timed(lambda: srv.score(cache, req_d, ns_c_d))
diff = max(float((p_full[t] - p_cached[t]).abs().max()) for t in cfg.tasks)
res = {
    'config': a.config, 'requests': Rq, 'candidates': C, 'L_S': cache.L_S, 'L_NS': cfg.num_ns_tokens,
    'full_forward': {'ms': round(t_full, 3), 'candidates_per_s': round(C / t_full * 1e3, 1)},
    'cached': {'ms': round(t_cached, 3), 'candidates_per_s': round(C / t_cached * 1e3, 1),
               'stage1_ms': round(t_s1, 3), 'stage2_ms': round(t_s2, 3)},
    'speedup': round(t_full / t_cached, 2), 'max_abs_prob_diff': diff}


def stats(xs):
    return {'median': round(float(np.median(xs)), 3), 'min': round(min(xs), 3), 'max': round(max(xs), 3)}


def extend_setup(dtypes):
    """Servers, events and times for the append measurement: this model, or its configuration without the pyramid."""
    m, note = model, a.config
    sched = srv.schedule(cache.L_S)
    if any(e['kS'] + e['kN'] < e['I'] for e in sched[:-1]):
        import copy
        flat = copy.deepcopy(cfg)
        flat.pyramid_enabled = False
        m, note = OneTransModel(flat, device=dev, seed=0), a.config + ' without pyramid'
    names = cfg.feature_config['sequence_features']
    new = torch.from_numpy(np.random.default_rng(3).integers(0, cfg.seq_item_vocab, (Rq, 4))).to(dev)
    times = None
    if getattr(cfg, 'seq_fusion', 'sep') == 'time':
        last = np.concatenate([seq_r[n + cfg.seq_time_suffix] for n in names], axis=1).max(axis=1)
        times = torch.from_numpy(last[:, None] + np.arange(1, 5)[None]).to(dev)
    return {k: OneTransServer(m, k) for k in dtypes}, note, names[-1], new, times


if a.cache_dtype != 'fp32':
    dtypes = ['fp32', 'bf16'] if a.cache_dtype == 'both' else [a.cache_dtype]
    servers = {k: OneTransServer(model, k) for k in dtypes}
    labels = {t: np.asarray(lab_c[t]).reshape(-1) for t in cfg.tasks}
    per = {k: {'stage1_ms': [], 'stage2_ms': []} for k in dtypes}
    esrv, enote, ename, enew, etimes = extend_setup(dtypes)
    ext = {k: {'reserve': [], 'no_reserve': []} for k in dtypes}
    with torch.no_grad():
        for _ in range(a.rounds):                            # alternate the dtypes inside the process
            for k in dtypes:
                t1, c = timed(lambda: servers[k].encode_requests(seq_r_d))
                t2, p = timed(lambda: servers[k].score(c, req_d, ns_c_d))
                per[k]['stage1_ms'].append(t1)
                per[k]['stage2_ms'].append(t2)
                per[k]['cache_bytes'] = c.nbytes()
                per[k]['max_abs_prob_diff'] = max(float((p_full[t] - p[t]).abs().max()) for t in cfg.tasks)
                per[k]['auc'] = {t: auc(labels[t], p[t].cpu().numpy()) for t in cfg.tasks}
                # append: a fresh encode outside the timed region each iteration would dominate, so the SAME cache is
                # extended every iteration — bf16 with reserve stays in place only the first time (later ones fork,
                # one copy), so the in-place figure times encode + extend and subtracts the encode
                for key, kw in (('reserve', {'reserve': 8} if k == 'bf16' else {}), ('no_reserve', {})):
                    te, _ = timed(lambda: esrv[k].encode_requests(seq_r_d, **kw))
                    tx, _ = timed(lambda: esrv[k].extend_requests(esrv[k].encode_requests(seq_r_d, **kw), ename, enew,
                                                                  etimes))
                    ext[k][key].append(tx - te)
    res['cache_dtypes'] = {k: {'stage1_ms': stats(v['stage1_ms']), 'stage2_ms': stats(v['stage2_ms']),
                               'cache_bytes': v['cache_bytes'], 'max_abs_prob_diff': v['max_abs_prob_diff'],
                               'auc': v['auc']} for k, v in per.items()}
    res['auc_full_forward'] = {t: auc(labels[t], p_full[t].cpu().numpy()) for t in cfg.tasks}
    res['extend_ms'] = {'config': enote, 'dL': 4,
                        **{k: {key: stats(v) for key, v in e.items()} for k, e in ext.items()}}
print(json.dumps(res))
