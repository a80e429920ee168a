"""ot_split_images alone: the one-launch build (ot_image_build 1) against the two-launch reference path (0) on the
image descriptors of the C2 and T flat layouts (no model: random weights in a buffer of the layout's size, the layout's
own descriptors, pair_dgrad as the split-mode model sets it), in alternating blocks within one process.  HIP events
bracket back-to-back runs of --calls calls after a warm-up; per layout it reports us per call of each (median and min
over the blocks), whether the two images are byte-equal, and the achieved GB/s against the build's byte floor: every
weight read once (4 B per element of every descriptor) plus the planes and column scales written.
    python tools/image_build_bench.py [--layouts C2 T] [--calls 50] [--rounds 7] [--mode split|bf16] [--out FILE.json]
    python tools/image_build_bench.py --once ref|new [--layouts C2]      one call per layout (for counter runs)
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommend_amd import kernels as K
from recommend_amd.config import workload_config
from recommend_amd.layout import IMAGE_UNIT_ELEMS, FlatLayout

ap = argparse.ArgumentParser()
ap.add_argument('--layouts', nargs='+', default=['C2', 'T'])
ap.add_argument('--calls', type=int, default=50, help='calls per timed block')
ap.add_argument('--rounds', type=int, default=7, help='alternations of the two builds')
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--mode', default='split', choices=['split', 'bf16'])
ap.add_argument('--once', default=None, choices=['ref', 'new'], help='one call of that build per layout, no timing')
ap.add_argument('--out', default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), 'image_build_bench needs the GPU (no CPU timing stands in for it)'
dev = torch.device('cuda', 0)
K.set_matmul_mode(args.mode)
SWITCH = {'ref': 0, 'new': 1}


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def floor_bytes(desc, one):
    """Weights read once per descriptor; planes (1 / 2 / 3 x 4 KiB per unit) and 516 B of scales per pair tile written."""
    rd = wr = 0
    for (_, _, _, _, ks, _, _, G, N, K_) in desc.tolist():
        tiles = G * ((N + 127) // 128)
        pair = not one and ks != -1
        rd += 4 * G * N * K_
        wr += tiles * (K_ // 16) * 4096 * (1 if one else 2 if pair else 3) + (516 * tiles if pair else 0)
    return rd, wr


def layout_times(name):
    cfg = workload_config(name)
    L = FlatLayout(cfg, cfg.ns_input_width(), pair_dgrad=args.mode == 'split')
    gen = torch.Generator(device='cpu').manual_seed(0)
    w = (0.05 * torch.randn(L.total, generator=gen)).to(dev)
    desc = torch.from_numpy(L.image_desc.reshape(-1)).to(dev)
    nd, units = L.image_desc.shape[0], L.image_units
    imgs = {k: torch.full((L.image_elems,), -23131, dtype=torch.int16, device=dev) for k in SWITCH}
    assert L.image_elems == units * IMAGE_UNIT_ELEMS

    def call(kind):
        K.image_build(SWITCH[kind])
        K.split_images(w, desc, nd, units, imgs[kind])

    rd, wr = floor_bytes(L.image_desc, args.mode == 'bf16')
    res = {'descriptors': int(nd), 'units': int(units), 'pair_descriptors': int((L.image_desc[:, 4] != -1).sum()),
           'tiles': int((L.image_desc[:, 7] * ((L.image_desc[:, 8] + 127) // 128)).sum()),
           'read_bytes': rd, 'write_bytes': wr}
    if args.once:
        call(args.once)
        torch.cuda.synchronize()
        return res

    def block(kind):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.calls):
            call(kind)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.calls

    for kind in SWITCH:
        for _ in range(args.warmup):
            call(kind)
    us = {k: [] for k in SWITCH}
    for _ in range(args.rounds):
        for kind in SWITCH:
            us[kind].append(block(kind))
    res['byte_equal'] = bool(torch.equal(imgs['ref'], imgs['new']))
    for kind in SWITCH:
        res[kind + '_us'] = stats(us[kind])
        res[kind + '_gbs'] = (rd + wr) / (float(np.median(us[kind])) * 1e-6) / 1e9
    res['new_median_below_ref_min'] = res['new_us']['median'] < res['ref_us']['min']
    return res


prev = K.image_build(-1)
res = {'device': torch.cuda.get_device_name(0), 'mode': args.mode, 'calls_per_block': args.calls,
       'rounds': args.rounds, 'once': args.once, 'layouts': {name: layout_times(name) for name in args.layouts}}
K.image_build(prev)
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
