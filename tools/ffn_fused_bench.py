"""C2's full-layer FFN forward (B 4096 x 140 tokens, d 128, f 512, split mode) as the two launches of the block forward
(FFN1: RMSNorm prologue, bias, row maxima, max |U|; FFN2: GELU prologue on the pair, bias, dropout, residual, rstd)
and as the fused kernel (ot_ffn_fused_fwd) with and without the U store.
HIP events, interleaved rounds, min / median per variant; U is compared bit for bit and x2 within the plane-vs-staged
tolerance.  `--once VARIANT` runs one variant three times (for a trace or PMC pass of its own).
Iteration tool; never part of the product path."""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from recommend_amd import kernels as K
from recommend_amd._lib import (OT_AX_GELU, OT_AX_RMSNORM, OT_EPI_BIAS, OT_EPI_DROPOUT, OT_EPI_RESIDUAL,
                                OT_EPI_ROW_RSTD, OT_GEMM_NT)
from recommend_amd.layout import IMAGE_UNIT_ELEMS

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--batch', type=int, default=4096)
ap.add_argument('--ffn', type=int, default=512)
ap.add_argument('--drop', type=float, default=0.1)
ap.add_argument('--once', default=None, help='run one variant only (two, fused+u, fused): profiling passes')
args = ap.parse_args()

dev = torch.device('cuda')
K.set_matmul_mode('split')
M, d, f = args.batch * 140, 128, args.ffn
ntiles = M // 128


def pair_image(W, gamma=None):
    G, N, K_ = W.shape
    base = torch.cat([W.reshape(-1), gamma if gamma is not None else torch.zeros(0)]).float().to(dev)
    desc = torch.tensor([0, K_, 1, N * K_, G * N * K_ if gamma is not None else -2, 0, 0, G, N, K_],
                        dtype=torch.int64, device=dev)
    units = G * (N // 128) * (K_ // 16)
    img = torch.zeros(units * IMAGE_UNIT_ELEMS, dtype=torch.int16, device=dev)
    K.split_images(base, desc, 1, units, img)
    return img


gen = torch.Generator().manual_seed(0)
tg = torch.zeros(ntiles, dtype=torch.int32, device=dev)
rows = torch.arange(M, dtype=torch.int32, device=dev)               # explicit row maps, as the model passes
x1 = torch.randn(M, d, device=dev)
rstd = torch.rsqrt((x1 * x1).mean(1) + 1e-6)
g = torch.rand(d, generator=gen) + 0.5
W1 = torch.randn(1, f, d, generator=gen) / math.sqrt(d)
W2 = torch.randn(1, d, f, generator=gen) / math.sqrt(f)
im1, im2 = pair_image(W1, g), pair_image(W2)
W1d, W2d, gd = W1.to(dev), W2.to(dev), g.to(dev)
b1, b2 = torch.randn(1, f, device=dev), torch.randn(1, d, device=dev)
u = torch.empty(M, f, device=dev)
umax = torch.empty(M, f // 128, device=dev)
x2, rstd_out = torch.empty(M, d, device=dev), torch.empty(M, device=dev)
amax = torch.zeros(1, device=dev)
dflag = OT_EPI_DROPOUT if args.drop > 0 else 0
tail = (140, 140)


def two():
    K.gemm_rms(OT_GEMM_NT, x1, d, d, rows, W1d, d * f, d, f, tg, ntiles, u, f, rows, epi=OT_EPI_BIAS,
               a_xform=OT_AX_RMSNORM, rstd=rstd, gamma=gd, bias=b1, bias_gstride=f, bimg=(im1, f // 128, 0),
               rowmax_out=umax, rowmax_n=f // 128, amax_out=amax, device=dev)
    K.gemm_rms(OT_GEMM_NT, u, f, f, rows, W2d, f * d, f, d, tg, ntiles, x2, d, rows, a_xform=OT_AX_GELU, bias=b2,
               bias_gstride=d, epi=OT_EPI_BIAS | OT_EPI_RESIDUAL | dflag | OT_EPI_ROW_RSTD, res=x1, ldres=d, res_tok=0,
               seed=7, site=1, drop=args.drop, tail=tail, rstd_out=rstd_out, eps=1e-6, bimg=(im2, 1, 0),
               a_rowmax=umax, a_rowmax_n=f // 128, device=dev)


def fused(with_u):
    K.ffn_fused_fwd(x1, d, rows, tg, ntiles, rstd, im1, 1, im2, 1, b1, f, b2, d, f, x2, d,
                    u_out=u if with_u else None, ldu=f, u_amax=amax, rstd_out=rstd_out, eps=1e-6, seed=7, site=1,
                    drop=args.drop, tail=tail)


variants = {'two': two, 'fused+u': lambda: fused(True), 'fused': lambda: fused(False)}
if args.once:
    variants = {args.once: variants[args.once]}
ref = None
for v, fn in variants.items():                                       # warm-up + agreement
    u.fill_(float('nan')); x2.fill_(float('nan'))
    fn(); fn(); fn()
    torch.cuda.synchronize()
    if ref is None:
        ref = (u.clone(), x2.clone())
    else:
        if v != 'fused':
            assert torch.equal(u.view(torch.int32), ref[0].view(torch.int32)), v
        torch.testing.assert_close(x2, ref[1], rtol=2e-5, atol=2e-5 * math.sqrt(f))
if args.once:
    sys.exit(0)
res = {v: [] for v in variants}
for _ in range(args.rounds):
    for v, fn in variants.items():
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); res[v].append(e0.elapsed_time(e1) * 1e3)
R = M * d * 4
print(f'rows {M} f {f} drop {args.drop}: R = rows x 128 x 4 B = {R / 1e9:.3f} GB')
for v in variants:
    print(f'{v:8s} min {min(res[v]):8.1f} us  median {float(np.median(res[v])):8.1f} us')
