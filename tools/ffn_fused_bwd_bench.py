"""C2's full-layer FFN input gradients (B 4096 x 140 tokens, d 128, f 512, split mode) as the two launches of the block
backward (FFN2 dgrad: GELU' epilogue, dU's row maxima and max |dU|; FFN1 dgrad: norm2 backward, residual gradient,
dropout mask, dgamma) and as the fused kernel (ot_ffn_fused_bwd).
HIP events, interleaved rounds, min / median per variant; dU is compared bit for bit and dx1 / dyo within the
plane-vs-staged tolerance.  `--once VARIANT` runs one variant three times (for a trace or PMC pass of its own).
`--mask-fused` times the FFN dropout's backward instead: {dropout pass + fused backward + W2 weight gradient} against
{fused backward masking dx2 itself (ot_ffn_fused_bwd_mask) + W2 weight gradient from its keep bits}, one stream, every
output compared bit for bit.
Iteration tool; never part of the product path."""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from recommend_amd import kernels as K
from recommend_amd._lib import (OT_AX_GELU, OT_EPI_DROPOUT, OT_EPI_GELU_BWD, OT_EPI_RMSNORM_BWD, OT_GEMM_NT,
                                OT_WG_D_KEEPBITS)
from recommend_amd.layout import IMAGE_UNIT_ELEMS, identity_map

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--batch', type=int, default=4096)
ap.add_argument('--ffn', type=int, default=512)
ap.add_argument('--drop', type=float, default=0.1)
ap.add_argument('--once', default=None, help='run one variant only (two, fused; pass, mask): profiling passes')
ap.add_argument('--mask-fused', action='store_true', help='the dropout pass against the in-kernel mask (drop > 0)')
args = ap.parse_args()

dev = torch.device('cuda')
K.set_matmul_mode('split')
M, d, f = args.batch * 140, 128, args.ffn
ntiles = M // 128


def pair_image(W):
    G, N, K_ = W.shape
    base = W.reshape(-1).float().to(dev)
    desc = torch.tensor([0, K_, 1, N * K_, -2, 0, 0, G, N, K_], dtype=torch.int64, device=dev)
    units = G * (N // 128) * (K_ // 16)
    img = torch.zeros(units * IMAGE_UNIT_ELEMS, dtype=torch.int16, device=dev)
    K.split_images(base, desc, 1, units, img)
    return img


gen = torch.Generator().manual_seed(0)
tg = torch.zeros(ntiles, dtype=torch.int32, device=dev)
rows = torch.arange(M, dtype=torch.int32, device=dev)               # explicit row maps, as the model passes
dy2 = torch.randn(M, d, device=dev)
dy2 = torch.where(torch.rand(M, d, device=dev) < args.drop, torch.zeros_like(dy2), dy2)   # as after the dropout pass
rm_dy2 = torch.empty(M, 1, device=dev)
K.rows_absmax(dy2, d, M, d, rm_dy2)
u = 1.5 * torch.randn(M, f, device=dev)
x1 = torch.randn(M, d, device=dev)
dx2 = torch.randn(M, d, device=dev)
rstd = torch.rsqrt((x1 * x1).mean(1) + 1e-6)
gamma = (torch.rand(d, generator=gen) + 0.5).to(dev)
W2 = torch.randn(1, f, d, generator=gen) / math.sqrt(f)             # the FFN2 dgrad's B[n = f][k = d]
W1 = torch.randn(1, d, f, generator=gen) / math.sqrt(d)             # the FFN1 dgrad's B[n = d][k = f]
im2, im1 = pair_image(W2), pair_image(W1)
W2d, W1d = W2.to(dev), W1.to(dev)
du = torch.empty(M, f, device=dev)
rm_du = torch.empty(M, f // 128, device=dev)
dx1, dyo = torch.empty(M, d, device=dev), torch.empty(M, d, device=dev)
rm_dyo = torch.empty(M, 1, device=dev)
dg = torch.zeros(d, device=dev)
b_du, b_dyo = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
dflag = OT_EPI_DROPOUT if args.drop > 0 else 0
tail = (140, 140)
dxm = dyo if args.drop > 0 else None


def two():
    K.gemm_rms(OT_GEMM_NT, dy2, d, d, rows, W2d, f * d, d, f, tg, ntiles, du, f, rows, epi=OT_EPI_GELU_BWD, aux=u,
               ldaux=f, bimg=(im2, f // 128, 0), amax_out=b_du, rowabs_out=rm_du, rowabs_n=f // 128, a_rowmax=rm_dy2,
               a_rowmax_n=1, device=dev)
    K.gemm_rms(OT_GEMM_NT, du, f, f, rows, W1d, d * f, f, d, tg, ntiles, dx1, d, rows, epi=OT_EPI_RMSNORM_BWD | dflag,
               seed=7, site=1, drop=args.drop, tail=tail, nx=x1, ldnx=d, ngamma=gamma, nrstd=rstd, dres=dx2, lddres=d,
               dx_masked=dxm, lddxm=d, dgamma=dg, device=dev, bimg=(im1, 1, 0), amax_out=b_dyo, rowabs_out=rm_dyo,
               rowabs_n=1, a_rowmax=rm_du, a_rowmax_n=f // 128)


def fused():
    K.ffn_fused_bwd(dy2, d, rm_dy2, 1, rows, tg, ntiles, im2, 1, im1, 1, f, u, f, du, f, x1, d, gamma, rstd, dx1, d, dg,
                    du_amax=b_du, dres=dx2, lddres=d, dx_masked=dxm, lddxm=d, amax_out=b_dyo, rowabs_out=rm_dyo,
                    rowabs_n=1, seed=7, site=1, drop=args.drop, tail=tail, device=dev)


variants = {'two': two, 'fused': fused}
if args.mask_fused:
    assert args.drop > 0
    imap = identity_map(M)
    cmap, nch = imap.to(dev), imap.chunks.shape[0]
    scale = float(np.float32(1) / (np.float32(1) - np.float32(args.drop)))
    dy2m, rm_m, b_m = torch.empty(M, d, device=dev), torch.empty(M, 1, device=dev), torch.zeros(1, device=dev)
    rm_x = torch.empty(M, 1, device=dev)
    K.rows_absmax(dx2, d, M, d, rm_x)                                # (the model: reported by dx2's producer)
    b_x, b_u = dx2.abs().max().reshape(1), u.abs().max().reshape(1)
    keep = torch.empty(M, d // 32, dtype=torch.int32, device=dev)
    dW2, db2 = torch.empty(1, f, d, device=dev), torch.empty(1, d, device=dev)
    wkw = dict(device=dev, a_bound=b_u, m_rows=M, rowmap=imap)

    def fused_on(a, rm, **kw):
        K.ffn_fused_bwd(a, d, rm, 1, rows, tg, ntiles, im2, 1, im1, 1, f, u, f, du, f, x1, d, gamma, rstd, dx1, d, dg,
                        du_amax=b_du, dres=dx2, lddres=d, dx_masked=dxm, lddxm=d, amax_out=b_dyo, rowabs_out=rm_dyo,
                        rowabs_n=1, seed=7, site=0, drop=args.drop, tail=tail, device=dev, **kw)

    def with_pass():
        K.dropout_apply(dx2, d, dy2m, d, M, d, 7, 1, args.drop, tail, amax=b_m, rowmax=rm_m)
        fused_on(dy2m, rm_m)
        K.wgrad(u, f, rows, dy2m, d, rows, f, d, cmap, nch, 1, dW2, f * d, db2, d, a_xform=OT_AX_GELU, d_bound=b_m, **wkw)

    def with_mask():
        fused_on(dx2, rm_x, mask_site=1, keep_out=keep, ldkeep=d // 32)
        K.wgrad(u, f, rows, dx2, d, rows, f, d, cmap, nch, 1, dW2, f * d, db2, d, a_xform=OT_AX_GELU | OT_WG_D_KEEPBITS,
                d_bound=b_x, keep=keep, ldkeep=d // 32, d_scale=scale, **wkw)

    variants = {'pass': with_pass, 'mask': with_mask}
    outs = lambda: [t.clone() for t in (du, dx1, dyo, dW2, db2)]
    with_pass(); torch.cuda.synchronize(); ref_m = outs()
    with_mask(); torch.cuda.synchronize()
    # the same binade of scale x bound in both paths wherever max |dx2| x scale rounds like max |dy2| (the kept
    # maximum): then every bit agrees; a row whose maximum was dropped has a finer scale in the pass path
    same = [torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs(), ref_m)]
    print('bitwise equal to the pass path (du, dx1, dyo, dW2, db2):', same)
    for a, b in zip(outs(), ref_m):
        torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-5 * math.sqrt(f))
if args.once:
    variants = {args.once: variants[args.once]}
ref = None
for v, fn in variants.items():                                       # warm-up + agreement
    du.fill_(float('nan')); dx1.fill_(float('nan')); dyo.fill_(float('nan'))
    fn(); fn(); fn()
    torch.cuda.synchronize()
    if args.mask_fused:
        continue                                                     # (compared above)
    if ref is None:
        ref = (du.clone(), dx1.clone(), dyo.clone())
    else:
        assert torch.equal(du.view(torch.int32), ref[0].view(torch.int32)), v
        torch.testing.assert_close(dx1, ref[1], rtol=2e-5, atol=2e-5 * math.sqrt(f))
        if dxm is not None:
            torch.testing.assert_close(dyo, ref[2], rtol=2e-5, atol=2e-5 * math.sqrt(f))
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
