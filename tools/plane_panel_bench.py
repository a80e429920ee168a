"""C2's three pair plane GEMM launches with several column tiles per row tile (FFN1 forward: RMSNorm prologue, bias,
row maxima; QKV forward: RMSNorm prologue; FFN2 dgrad: plain A with row bounds, GELU' epilogue, row bounds out) at
B 4096 x 140 tokens, d 128, f 512, under the kernel switches: row metadata from the row maps / parked in LDS
(ot_plane_rowmeta 0 / 1) on the one-tile kernel, and the panel form (ot_plane_panel) at widths 2 / ntn and auto, on its three-
and four-workgroups-per-CU variants and with A's fragments held across the column tiles.
HIP events, interleaved rounds, min / median per variant; every variant's outputs are compared bit for bit with the
first one's.  `--once VARIANT` runs each launch three times under one variant (for a PMC or trace pass of its own).
Iteration tool; never part of the product path."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from recommend_amd import kernels as K
from recommend_amd._lib import OT_GEMM_NT, OT_AX_NONE, OT_AX_RMSNORM, OT_EPI_BIAS, OT_EPI_GELU_BWD
from recommend_amd.layout import IMAGE_UNIT_ELEMS

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--batch', type=int, default=4096)
ap.add_argument('--once', default=None, help='run one variant only (e.g. old, meta, panel): profiling passes')
args = ap.parse_args()

dev = torch.device('cuda')
K.set_matmul_mode('split')
M, d, f = args.batch * 140, 128, 512
ntiles = M // 128


def pair_image(W, gamma=None):
    G, N, K_ = W.shape
    base = torch.cat([W.reshape(-1), gamma if gamma is not None else torch.zeros(0)]).float().to(dev)
    desc = torch.tensor([0, K_, 1, N * K_, G * N * K_ if gamma is not None else -2, 0, 0, G, N, K_],
                        dtype=torch.int64, device=dev)
    units = G * (N // 128) * (K_ // 16)
    img = torch.zeros(units * IMAGE_UNIT_ELEMS, dtype=torch.int16, device=dev)
    K.split_images(base, desc, 1, units, img)
    return img, N // 128


gen = torch.Generator().manual_seed(0)
tg = torch.zeros(ntiles, dtype=torch.int32, device=dev)
rows = torch.arange(M, dtype=torch.int32, device=dev)               # explicit row maps, as the model passes
x = torch.randn(M, d, device=dev)
rstd = torch.rsqrt((x * x).mean(1) + 1e-6)
g = torch.rand(d, generator=gen) + 0.5
im1, n1 = pair_image(torch.randn(1, f, d, generator=gen) * 0.1, g)
imq, nq = pair_image(torch.randn(1, 3 * d, d, generator=gen) * 0.1, g)
im2, n2 = pair_image(torch.randn(1, f, d, generator=gen) * 0.1)    # FFN2 dgrad: B[n = f][k = d]
b1 = torch.randn(1, f, device=dev)
u = torch.empty(M, f, device=dev); qkv = torch.empty(M, 3 * d, device=dev); du = torch.empty(M, f, device=dev)
rmax = torch.empty(M, f // 128, device=dev); rabs = torch.empty(M, f // 128, device=dev)
amax = torch.zeros(1, device=dev)
dy = torch.randn(M, d, device=dev); dymax = dy.abs().amax(1, keepdim=True).contiguous()
Wd = torch.zeros(4, device=dev); gd = g.to(dev)
cases = {
    'ffn1 fwd': (lambda: K.gemm_rms(OT_GEMM_NT, x, d, d, rows, Wd, 0, d, f, tg, ntiles, u, f, rows, epi=OT_EPI_BIAS,
                                    a_xform=OT_AX_RMSNORM, rstd=rstd, gamma=gd, bias=b1, bias_gstride=f,
                                    bimg=(im1, n1, 0), rowmax_out=rmax, rowmax_n=f // 128, device=dev), (u, rmax)),
    'qkv fwd': (lambda: K.gemm(OT_GEMM_NT, x, d, d, rows, Wd, 0, d, 3 * d, tg, ntiles, qkv, 3 * d, rows,
                               a_xform=OT_AX_RMSNORM, rstd=rstd, gamma=gd, bimg=(imq, nq, 0)), (qkv,)),
    'ffn2 dgrad': (lambda: K.gemm_rms(OT_GEMM_NT, dy, d, d, rows, Wd, 0, d, f, tg, ntiles, du, f, rows,
                                      epi=OT_EPI_GELU_BWD, a_xform=OT_AX_NONE, aux=u, ldaux=f, a_rowmax=dymax,
                                      a_rowmax_n=1, rowabs_out=rabs, rowabs_n=f // 128, amax_out=amax,
                                      bimg=(im2, n2, 0), device=dev), (du, rabs)),
}
# variant -> (ot_plane_rowmeta, ot_plane_panel)
variants = {'old': (0, 0), 'meta': (1, 0), 'panel w2': (1, 2), 'panel w4': (1, 4), 'panel': (1, 1),
            'panel4cu w2': (1, 102), 'panel4cu w4': (1, 104), 'holdA w4': (1, 204)}
HAVE = hasattr(K, 'plane_panel')             # (a library from before the switches: the one-tile kernel only)
if not HAVE:
    variants = {'old': (0, 0)}
if args.once:
    variants = {args.once: variants[args.once]}


def setv(v):
    if HAVE:
        K.plane_rowmeta(variants[v][0]); K.plane_panel(variants[v][1])


ref = {}
for v in variants:                                                   # warm-up + bit-identity
    setv(v)
    for k, (fn, outs) in cases.items():
        fn(); fn(); fn()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        if k not in ref:
            ref[k] = got
        else:
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ref[k], got)), (v, k)
if args.once:
    sys.exit(0)
res = {(v, k): [] for v in variants for k in cases}
for _ in range(args.rounds):
    for v in variants:
        setv(v)
        for k, (fn, _o) in cases.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize(); res[(v, k)].append(e0.elapsed_time(e1) * 1e3)
print(f'{"variant":12s} ' + ' '.join(f'{k + " min/med us":>24s}' for k in cases))
for v in variants:
    print(f'{v:12s} ' + ' '.join(f'{min(res[(v, k)]):11.1f} /{float(np.median(res[(v, k)])):10.1f}' for k in cases))
