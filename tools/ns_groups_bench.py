"""Group-wise NS tokenizer (ns_tokenizer='group'; ot_ns_group_fwd / _bwd_input / _bwd_weight) against the auto-split
tokenizer it replaces, at C2: B = 4096, F_ns = 429, L_NS = 12, d = 128, groups from config.even_ns_groups.

    python3 tools/ns_groups_bench.py [--rounds 30] [--steps 20] [--warmup 5] [--out FILE.json]

1. kernels   each grouped kernel against the auto-split launch of the same role (the tokenizer's forward GEMM, its
             dns GEMM and its weight gradient, called as model._Tokenize calls them), on resident random data: HIP
             events around each call, a synchronise after it, the two sides alternated inside every round, medians.
2. forward   the grouped forward's compulsory bytes (B * f_pad * 4 read + B * L_NS * d * 4 written) over its time,
             against the device copy rate measured here (tools/hbm_calib.py's 1 GiB copy).
3. step      a whole C2 train_step with 'group' against 'auto': two models of one seed, resident batches, alternating
             steps, medians and spread.
Prints one JSON line per measurement; ``--out`` also writes them as one JSON list.
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
ap.add_argument('--rounds', type=int, default=30)
ap.add_argument('--steps', type=int, default=20, help='timed train steps per side (0 = skip the step comparison)')
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--out', default='')
a = ap.parse_args()

dev = torch.device('cuda')


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
    n = (1 << 30) // 4
    x = torch.empty(n, device=dev).uniform_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    ms = [timed(lambda: y.copy_(x))[0] for _ in range(10)]
    return 2.0 * n * 4 / (1e-3 * float(np.median(ms)))


def configs():
    from recommend_amd.config import even_ns_groups, workload_config
    auto = workload_config('C2')
    group = copy.deepcopy(auto)
    group.ns_tokenizer, group.ns_token_groups = 'group', even_ns_groups(group)
    return auto, group


def bench_kernels(hbm):
    from recommend_amd import kernels as K
    from recommend_amd._lib import OT_EPI_BIAS, OT_GEMM_NT
    from recommend_amd.model import OneTransModel
    cfg_a, cfg_g = configs()
    B, d, L = cfg_a._batch, cfg_a.hidden_dim, cfg_a.num_ns_tokens
    ma, mg = OneTransModel(cfg_a, device=dev, seed=0), OneTransModel(cfg_g, device=dev, seed=0)
    F, fp = ma.f_ns, ma.layout.f_pad
    nsm = torch.zeros(B, fp, device=dev)
    nsm[:, :F].normal_()
    x0 = torch.empty(B * L, d, device=dev)
    dx0 = torch.empty(B * L, d, device=dev).normal_()
    dns = torch.empty(B, fp, device=dev)
    rm = ma.ident_rows(B)
    mp = rm.to(dev)
    Lnsd = L * d
    with K.precision(ma.matmul):
        fns = {
            'fwd': {
                'auto': lambda: K.gemm(OT_GEMM_NT, nsm, fp, fp, mp['rows'][0], ma.pT('tok.ns.kernel'), 0, fp, Lnsd,
                                       mp['tile_group'], rm.ntiles, x0, Lnsd, mp['rows'][0],
                                       bias=ma.p('tok.ns.bias'), epi=OT_EPI_BIAS, m_rows=B,
                                       bimg=ma.bimg('tok.ns.kernel')),
                'group': lambda: K.ns_group_fwd(nsm, fp, mg.ns_goff, L, fp, mg.ns_kmax, mg.p('tok.ns.kernel'),
                                                mg.p('tok.ns.bias'), B, d, x0, Lnsd)},
            'bwd_input': {
                'auto': lambda: K.gemm(OT_GEMM_NT, dx0, Lnsd, Lnsd, mp['rows'][0], ma.p('tok.ns.kernel'), 0, Lnsd, fp,
                                       mp['tile_group'], rm.ntiles, dns, fp, mp['rows'][0], m_rows=B),
                'group': lambda: K.ns_group_bwd_input(dx0, Lnsd, mg.ns_goff, L, fp, mg.ns_kmax, mg.p('tok.ns.kernel'),
                                                      B, d, dns, fp)},
            'bwd_weight': {
                'auto': lambda: K.wgrad(nsm, fp, mp['rows'][0], dx0, Lnsd, mp['rows'][0], fp, Lnsd, mp,
                                        rm.chunks.shape[0], 1, ma.g('tok.ns.kernel'), 0, ma.g('tok.ns.bias'), 0,
                                        device=dev, m_rows=B, rowmap=rm),
                'group': lambda: K.ns_group_bwd_weight(nsm, fp, dx0, Lnsd, mg.ns_goff, L, fp, mg.ns_kmax, B, d,
                                                       mg.g('tok.ns.kernel'), mg.g('tok.ns.bias'), device=dev)},
        }
        for pair in fns.values():
            for fn in pair.values():
                for _ in range(3):
                    fn()
        torch.cuda.synchronize()
        ms = {k: {s: [] for s in pair} for k, pair in fns.items()}
        for r in range(a.rounds):
            for k, pair in fns.items():
                for s in (('auto', 'group') if r % 2 == 0 else ('group', 'auto')):
                    ms[k][s].append(timed(pair[s])[0])
    out = []
    for k, sides in ms.items():
        med = {s: float(np.median(v)) for s, v in sides.items()}
        out.append({'kernel': k, 'B': B, 'F_ns': F, 'L_NS': L, 'd': d, 'rounds': a.rounds, 'matmul': ma.matmul,
                    'us': {s: round(1e3 * v, 2) for s, v in med.items()},
                    'min_us': {s: round(1e3 * float(np.min(v)), 2) for s, v in sides.items()},
                    'group_over_auto': round(med['group'] / med['auto'], 4),
                    'flops': {'auto': 2.0 * B * F * L * d, 'group': 2.0 * B * F * d}})
    fwd = float(np.median(ms['fwd']['group']))
    nbytes = B * fp * 4 + B * L * d * 4
    rate = nbytes / (1e-3 * fwd)
    out.append({'forward_bytes': nbytes, 'what': 'B*f_pad*4 read + B*L_NS*d*4 written over the grouped forward time',
                'GBps': round(rate / 1e9, 1), 'over_copy_rate': round(rate / hbm, 4)})
    return out


def bench_step():
    from recommend_amd.data import make_batch
    from recommend_amd.model import OneTransModel
    from recommend_amd.trainer import OneTransTrainer
    cfg_a, cfg_g = configs()
    B = cfg_a._batch
    batches = [tuple(to_dev(p) for p in make_batch(B, cfg_a, seed=100 + i)) for i in range(4)]
    tr = {m: OneTransTrainer(c, model=OneTransModel(c, device=dev, seed=0)) for m, c in (('auto', cfg_a), ('group', cfg_g))}
    ms = {m: [] for m in tr}
    for step in range(a.warmup + a.steps):
        for m in (('auto', 'group') if step % 2 == 0 else ('group', 'auto')):
            dt, out = timed(lambda: tr[m].train_step(batches[step % 4]))
            if step >= a.warmup and bool(torch.isfinite(out['total_loss'])):
                ms[m].append(dt)
    med = {m: float(np.median(v)) for m, v in ms.items()}
    return {'train_step': 'C2', 'B': B, 'steps': a.steps, 'auto_ms': round(med['auto'], 3),
            'group_ms': round(med['group'], 3), 'group_over_auto': round(med['group'] / med['auto'], 4),
            'spread_ms': {m: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for m, v in ms.items()}}


def main():
    res = []
    hbm = copy_rate()
    res.append({'copy_rate_GBps': round(hbm / 1e9, 1), 'what': '1 GiB device copy, read + write bytes over time'})
    print(json.dumps(res[-1]), flush=True)
    for r in bench_kernels(hbm):
        res.append(r)
        print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    if a.steps:
        res.append(bench_step())
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
