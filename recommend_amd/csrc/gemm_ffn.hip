// The fused FFN forward of the split mode at d = 128 (ot_ffn_fused_fwd): x2 = x1 + drop(gelu(norm2(x1) W1 + b1) W2 + b2)
// in one kernel, U = norm2(x1) W1 + b1 never read back from memory (written only when the caller wants it).
// And its backward (ot_ffn_fused_bwd, further down): the FFN2 dgrad, GELU' and the FFN1 dgrad with the norm2 backward in
// one kernel, dU written once and not read back.
#include <atomic>
#include <cstdlib>
#include <mutex>

#include "gemm.h"

namespace ot {

// One workgroup of 4 waves per 128-row tile, wave w owning rows 32w .. 32w+31 for the whole tile (plane_gemm_kernel's
// 4x1 layout, the same row maps, weight group, rstd-bound A scale and global_load_lds stage ring).  For each
// 128-column chunk c of f:
//   1. GEMM1, transposed: acc1[nb] = mfma(W1 image fragment as A, x1 pair fragment as B) — plane_gemm_kernel's two
//      fragments with the MFMA's operand roles swapped, the same three products in the same order over the same k, so
//      acc1 is U^T bit for bit: lane li = x1 row, register r = f index 32 nb + (r & 3) + 8 (r >> 2) + 4 h.
//   2. U finished in registers: unscale (row factor per lane, column factor per register), rstd, bias — the operations
//      of the unfused TERMS-2 unscale and gemm_vec_epilogue<OT_EPI_BIAS> with ROWSCALE in their order; the chunk's
//      signed row maximum (in-lane, one exchange between the lane halves) and max |U| (the W2 weight gradient's bound).
//   3. U to memory when u_out is given: a wave-private LDS transposer (32 rows x 32 columns per pass), 128-B row runs,
//      the non-temporal stores of store_out4.
//   4. GEMM2 from the accumulators: h = gelu(U) pair-split with this chunk's row scale pow2_scale14(max(rowmax, 0.17));
//      registers 8s .. 8s+7 of acc1[nb] are the B fragment of k-step 2 nb + s of the chunk, whose element j of lane
//      half h is f offset 8 (j >> 2) + 4 h + (j & 3): the W2 fragment is read as two 8-byte halves of the image's
//      16-k row.  acc2 carries the current chunk's scale: before a chunk's products it is multiplied by s_c / s_(c-1)
//      (a power of two: exact), and unscaled by the last s_c at the end.  No chunk's scale is coarser than the
//      unfused launch's row-wide one.
// After the last chunk acc2 (lane = row: LAYOUT 5 of gemm_vec_epilogue) runs FFN2's epilogue unchanged.
//
// Stages (16 KiB each, FF_NST in the ring): a chunk is 8 GEMM1 stages (16 k of x1's rows, re-streamed per chunk as the
// four column-tile workgroups of the unfused launch do, + 16 k of W1's column tile c) and 4 GEMM2 stages (32 k = two
// units of W2's image): 4 copies per wave either way, so with three buffers a stage is waited for with vmcnt(4) while
// the next one's copies fly (measured: within 3% of the two-buffer ring, steadier).  The wait after the U stores (a
// chunk's first GEMM2 stage) and the last one are vmcnt(0): no counted wait has a store in flight.
#ifndef OT_FFN_NSTG
#define OT_FFN_NSTG 3
#endif
constexpr int FF_NST = OT_FFN_NSTG;
static_assert(FF_NST == 2 || FF_NST == 3, "fused FFN stage buffers");
constexpr int PG_A_BYTES = GT * 16 * 4;                     // A stage image: 128 rows x 16 f32 (as gemm_plane.hip's)
constexpr int FF_STG = PG_A_BYTES + 2 * GT * 16 * 2;       // 16 KiB
constexpr int FF_TR_LD = 36;                                // transposer row stride (floats): 32 columns + 4
constexpr int FF_TR_WAVE = 32 * FF_TR_LD * 4;               // one wave's transposer (4,608 B)
constexpr int FF_TR_OFF = FF_NST * FF_STG;
constexpr int FF_META_OFF = FF_TR_OFF + 4 * FF_TR_WAVE;     // 128 output rows (gemm_vec_epilogue's rmeta)
constexpr int FF_TAB_OFF = FF_META_OFF + GT * 4;            // f column factors of W1's image, f of b1, 128 of W2's
constexpr int FF_MAX_F = 1024;                              // two workgroups per CU: 80 KiB each
static_assert(FF_META_OFF >= (64 * (GT + 4) + 8 * GT) * 4, "fused FFN: the epilogue tile overlays the row metadata");
static_assert(FF_TAB_OFF + (2 * FF_MAX_F + GT) * 4 <= 80 * 1024, "fused FFN LDS");
constexpr int ffn_lds(int f) { return FF_TAB_OFF + (2 * f + GT) * 4; }

struct FfnArgs {
  GemmArgs e;                         // FFN2's epilogue operands; A / lda / in_rows / a_rstd / K: x1 and norm2's rstd
  const uint16_t* img1; int g1;       // W1 forward image (pair form, gamma folded); g1: one image per weight group
  const uint16_t* img2; int g2;       // W2 forward image (pair form)
  const float* b1; int64_t b1_gstride;
  float* u_out; int64_t ldu;
  float* u_amax;
  int f;
};

// (W operand as the MFMA's A: the three products of mfma_pair(x, w) in its order)
__device__ __forceinline__ f32x16 mfma_pair_t(const u32x4 (&w)[2], const u32x4 (&x)[3], f32x16 c) {
  c = mfma_f16(w[1], x[0], c);
  c = mfma_f16(w[0], x[1], c);
  return mfma_f16(w[0], x[0], c);
}

template <int EPIT>
__global__ __launch_bounds__(256, 2) void ffn_fused_kernel(FfnArgs q) {
  const GemmArgs& p = q.e;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int tm = xcd_remap(blockIdx.x, p.ntm);
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int nch = q.f >> 7;

  // stage copies as plane_panel_kernel's (A: wave w's instruction i fills KiB 2w + i of the A image)
  const float* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (2 * wave + i) * 16 + (lane >> 2);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    const int lc = (lane & 3) ^ ((r >> 2) & 3);
    asrc[i] = p.A + (int64_t)ir * p.lda + 4 * lc;
  }
  constexpr int64_t T1 = 8 * (int64_t)PG_B_BYTES;             // one W1 column tile: K = 128 = 8 units
  const char* img1 = reinterpret_cast<const char*>(q.img1) + (int64_t)(q.g1 ? g : 0) * nch * T1;
  const char* img2 = reinterpret_cast<const char*>(q.img2) + (int64_t)(q.g2 ? g : 0) * (q.f >> 4) * PG_B_BYTES;
  const int blane = 2 * wave * 1024 + 16 * lane;
  auto issue = [&](int c, int sidx, int buf) {
    char* sb = lds + buf * FF_STG;
    if (sidx < 8) {
      const char* bs = img1 + c * T1 + (int64_t)sidx * PG_B_BYTES + blane;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + 16 * sidx), (lds_void_t*)(sb + (2 * wave + i) * 1024),
                                         16, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(bs + i * 1024),
                                         (lds_void_t*)(sb + PG_A_BYTES + (2 * wave + i) * 1024), 16, 0, 0);
    } else {
      const char* bs = img2 + (int64_t)(8 * c + 2 * (sidx - 8)) * PG_B_BYTES + blane;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_global_load_lds((const void*)(bs + u * PG_B_BYTES + i * 1024),
                                           (lds_void_t*)(sb + u * 8192 + (2 * wave + i) * 1024), 16, 0, 0);
    }
  };

  const int ra = 32 * wave + li;                      // this lane's row of the tile
  const int aoff0 = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
  const int aoff1 = ra * 64 + 16 * ((2 * h + 1) ^ ((li >> 2) & 3));
  const int sw = (li >> 3) & 1;
  const int boff = PG_A_BYTES + li * 32 + 16 * (h ^ sw);
  const int woff0 = li * 32 + 16 * sw + 8 * h;        // W2: k 4h .. 4h+3 and 8 + 4h .. of the unit's 16
  const int woff1 = li * 32 + 16 * (1 ^ sw) + 8 * h;

  // the row's rstd (A scale bound and row factor) and output row
  float abound;
  int mrow;
  bool mok;
  {
    const int64_t gr = (int64_t)tm * GT + ra;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    mok = ir >= 0;
    mrow = p.out_rows ? p.out_rows[gr] : (int)gr;
    abound = p.a_rstd[ir < 0 ? 0 : ir];
  }
  // W1's column factors (1 / s_n, NaN for an image without the pair tag) and b1, once per tile
  float* tab = reinterpret_cast<float*>(lds + FF_TAB_OFF);
  for (int idx = t; idx < q.f; idx += 256) {
    const float* cs = reinterpret_cast<const float*>(img1 + (idx >> 7) * T1 + 2 * GT * 16 * 2);
    const float bad = reinterpret_cast<const uint32_t*>(cs)[GT] == PAIR_IMAGE_TAG ? 1.f : __builtin_nanf("");
    tab[idx] = bad / cs[idx & 127];
    tab[q.f + idx] = q.b1[(int64_t)g * q.b1_gstride + idx];
  }
  if (t < GT) {                                       // W2's column factors
    const float* cs = reinterpret_cast<const float*>(img2 + 2 * GT * 16 * 2);
    const float bad = reinterpret_cast<const uint32_t*>(cs)[GT] == PAIR_IMAGE_TAG ? 1.f : __builtin_nanf("");
    tab[2 * q.f + t] = bad / cs[t];
  }
  int* rmeta = reinterpret_cast<int*>(lds + FF_META_OFF);
  if (h == 0) rmeta[ra] = mrow;
  const float asc = pow2_scale14(sqrtf((float)p.K) / abound);
  const float ainv = 1.f / asc;
  const float rsc = mok ? abound : 0.f;
  float* trw = reinterpret_cast<float*>(lds + FF_TR_OFF + wave * FF_TR_WAVE);
  // every load above is waited for here, before the first copy is in flight: the empty statement reads their
  // registers, so no wait for them can sink into the main loop (where it would drain the stage copies)
  asm volatile("" : "+v"(abound), "+v"(mrow));

  issue(0, 0, 0);
  if (FF_NST == 3) issue(0, 1, 1);
  f32x16 acc2[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[a][r] = 0.f;
  float am = 0.f, hsc = 1.f, hinv = 1.f;

  for (int c = 0; c < nch; ++c) {
    // stage (c, sidx) has landed (every wave's after the barrier); the barrier also retires the reads of the buffer
    // that the next stage's copies then overwrite
    auto top = [&](int sidx) {
      if (FF_NST == 2 || sidx == 8 || (sidx == 11 && c + 1 == nch)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      constexpr int AH = FF_NST - 1;                    // the stage copied now: AH ahead, into the buffer read last
      if (sidx + AH < 12) issue(c, sidx + AH, (sidx + AH) % FF_NST);       // in the iteration before this barrier
      else if (c + 1 < nch) issue(c + 1, sidx + AH - 12, (sidx + AH) % FF_NST);
    };
    f32x16 acc1[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[a][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      top(kt);
      const char* sb = lds + (kt % FF_NST) * FF_STG;
      u32x4 fb[4][2];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) fb[nb][pl] = *reinterpret_cast<const u32x4*>(sb + boff + pl * 4096 + nb * 1024);
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + aoff1);
      const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      u32x4 fa[3];
      pair8(av, asc, fa);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc1[nb] = mfma_pair_t(fb[nb], fa, acc1[nb]);
    }
    // ---- U of this chunk, in registers
    float mx = -__builtin_inff(), ua = 0.f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int fo = 128 * c + 32 * nb + 8 * qd + 4 * h;
        const f32x4 ci = *reinterpret_cast<const f32x4*>(tab + fo);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(tab + q.f + fo);
        f32x4 v = {acc1[nb][4 * qd], acc1[nb][4 * qd + 1], acc1[nb][4 * qd + 2], acc1[nb][4 * qd + 3]};
        v = v * (ainv * ci);
        v = v * rsc;
        v += bb;
        mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        ua = amax4(ua, v);
        acc1[nb][4 * qd] = v.x; acc1[nb][4 * qd + 1] = v.y; acc1[nb][4 * qd + 2] = v.z; acc1[nb][4 * qd + 3] = v.w;
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (mrow >= 0) am = fmaxf(am, ua);
    {
      const float s = pow2_scale14(fmaxf(mx, 0.17f));
      if (c > 0) {
        const float ratio = s * hinv;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc2[a][r] *= ratio;
      }
      hsc = s;
      hinv = 1.f / s;
    }
    if (q.u_out) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
          *reinterpret_cast<f32x4*>(trw + li * FF_TR_LD + 8 * qd + 4 * h) =
              f32x4{acc1[nb][4 * qd], acc1[nb][4 * qd + 1], acc1[nb][4 * qd + 2], acc1[nb][4 * qd + 3]};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's writes before its reads
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(trw + ((lane >> 3) + 8 * ps) * FF_TR_LD + 4 * (lane & 7));
          const int ur = rmeta[32 * wave + (lane >> 3) + 8 * ps];     // (published by the main loop's barriers)
          if (ur >= 0) store_out4(q.u_out + (int64_t)ur * q.ldu + 128 * c + 32 * nb + 4 * (lane & 7), v);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // rewritten by the next pass
      }
    }
    // ---- GEMM2: acc1[j] is the B operand of the chunk's units 2j, 2j + 1
    auto stage2 = [&](int j, const f32x16& u) {
      top(8 + j);
      const char* sb = lds + ((8 + j) % FF_NST) * FF_STG;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f32x4 g0 = gelu_erf4(f32x4{u[8 * s], u[8 * s + 1], u[8 * s + 2], u[8 * s + 3]});
        const f32x4 g1 = gelu_erf4(f32x4{u[8 * s + 4], u[8 * s + 5], u[8 * s + 6], u[8 * s + 7]});
        const float hv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        u32x4 fh[3];
        pair8(hv, hsc, fh);
        u32x4 fw[4][2];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) {
            const char* wb = sb + s * 8192 + pl * 4096 + nb * 1024;
            const u32x2 lo = *reinterpret_cast<const u32x2*>(wb + woff0);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(wb + woff1);
            fw[nb][pl] = u32x4{lo.x, lo.y, hi.x, hi.y};
          }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc2[nb] = mfma_pair_t(fw[nb], fh, acc2[nb]);
      }
    };
    stage2(0, acc1[0]);
    stage2(1, acc1[1]);
    stage2(2, acc1[2]);
    stage2(3, acc1[3]);
  }
  // unscale: the last chunk's row scale (per lane), W2's column factors (per register)
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const f32x4 cs = *reinterpret_cast<const f32x4*>(tab + 2 * q.f + 32 * nb + 8 * qd + 4 * h);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc2[nb][4 * qd + i] *= hinv * cs[i];
    }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                    // the epilogue reuses the stage buffers
  gemm_vec_epilogue<EPIT, 5, false, 8, false>(p, acc2, smem, tm, 0, g, 0, -1, rmeta);
  if (q.u_amax) amax_flush(q.u_amax, am);             // (uniform: every wave reaches it)
}

// 1 = the model's FFN forward takes ot_ffn_fused_fwd where its form applies, 0 = the FFN1 and FFN2 launches; the
// environment variable ONETRANS_FFN_FUSED (0 / 1) sets the process's initial value
#ifndef OT_FFN_FUSED
#define OT_FFN_FUSED 1
#endif
static int ffn_fused_initial() {
  const char* e = getenv("ONETRANS_FFN_FUSED");
  return e && *e ? (atoi(e) != 0) : OT_FFN_FUSED;
}
static std::atomic<int> g_ffn_fused{ffn_fused_initial()};

// ---- The fused FFN backward of the split mode at d = 128 (ot_ffn_fused_bwd): the FFN2 dgrad dU = (dy2 W2^T) gelu'(u)
// and the FFN1 dgrad dx1 = norm2_bwd(dU W1^T) + dx2 in one kernel, dU written once (the W1 weight gradient and db1 read
// it) and never read back, no row maxima of dU through memory.
//
// ffn_fused_kernel's structure: the same row maps, weight group, xcd_remap, stage ring and lane = row layouts.  For
// each 128-column chunk c of f:
//   1. GEMM1, transposed: acc1[nb] = mfma(W2 dgrad image fragment as A, dy2 pair fragment as B): the three products of
//      plane_gemm_kernel<OT_AX_NONE, OT_EPI_GELU_BWD, .., 2> in its order over the same k, dy2's row scale from the
//      a_rowmax parts that launch is given: acc1 is that launch's accumulator tile, transposed, bit for bit.
//   2. dU finished in registers, 32 columns per u stage: the unscale (row factor per lane, column factor per register)
//      times gelu_erf_grad4(u) — the unfused unscale and OT_EPI_GELU_BWD epilogue in their order — with u read from the
//      stage ring (lane = row reads of 16 B; the copies place the 16-B piece j of row r at j ^ ((r >> 1) & 7) of the
//      row's 128 B, so 16 consecutive rows cover the 64 banks once); the chunk's row maximum of |dU| and max |dU| (the
//      W1 weight gradient's bound).
//   3. dU to memory through the wave-private transposer, as the forward stores U.
//   4. GEMM2 from the accumulators: dU pair-split with the row scale of this chunk, the W1 dgrad image read as the two
//      8-byte halves that match the accumulators' k order.  A chunk's scale is pow2_scale14 of the largest |dU| of the
//      row's chunks so far: never coarser than the unfused launch's row-wide one, and it only ever shrinks, so the
//      running sums' factor s_c / s_(c-1) is a power of two <= 1 (a factor > 1 — a small chunk after a large one —
//      could overflow them).  A row of zeros has scale 1.
// After the last chunk acc2 (LAYOUT 5) runs the FFN1 dgrad's OT_EPI_RMSNORM_BWD [| OT_EPI_DROPOUT] epilogue unchanged.
//
// Stages (16 KiB, FF_NST in the ring, 4 copies per wave each): a chunk is 8 GEMM1 stages (16 k of dy2's rows + 16 k of
// W2's column tile c), 4 u stages (128 rows x 32 columns) and 4 GEMM2 stages (two units of W1's image).  16 stages do
// not divide by three, so the ring position is carried (a scalar), not derived from the stage index.  The wait after
// the dU stores (a chunk's first GEMM2 stage) and the last one are vmcnt(0).
constexpr int FB_TAB_OFF = FF_TAB_OFF;                      // f column factors of W2's image, 128 of W1's
constexpr int FB_KEEP_BYTES = GT * (GT / 8);                // the mask mode's keep bits: 16 B per row, after the factors
static_assert(FB_TAB_OFF + (FF_MAX_F + GT) * 4 + FB_KEEP_BYTES <= 80 * 1024, "fused FFN backward LDS");
constexpr int ffn_bwd_lds(int f, bool mask = false) { return FB_TAB_OFF + (f + GT) * 4 + (mask ? FB_KEEP_BYTES : 0); }

struct FfnBwdArgs {
  GemmArgs e;                         // FFN1 dgrad's epilogue operands; A / lda / in_rows / a_rowmax: dy2 and its maxima
  const uint16_t* img2; int g2;       // W2 dgrad image (pair form: f / 128 column tiles of 8 units per group)
  const uint16_t* img1; int g1;       // W1 dgrad image (pair form: f / 16 units per group)
  const float* u; int64_t ldu;
  float* du; int64_t lddu;
  float* du_amax;
  int f;
  // MASKA: A is dx2, the gradient before the FFN dropout's mask; dy2 = keep ? dx2 * e.drop_scale : 0 is formed at
  // fragment time from (e.seed, a_site, e.drop_thr, e's tail map), and the keep bits go to keep_out
  uint32_t a_site; uint32_t* keep_out; int64_t ldkeep;
};

// MASKA (ot_ffn_fused_bwd_mask): the stage copies stay raw copies of the A rows.  In the prologue each lane hashes the
// 64 columns of its row that it will read (k = 16 kt + 8 h + e: byte 2 kt + h of the row's 16, so the table is the
// row's bits in column order) into an LDS table; a k-step reads its byte back and selects (nothing more is held across
// the loop: the kernel sits at the register cap).  The values are dropout_apply_kernel's: the same index, the same
// f32 multiply.
template <int EPIT, bool MASKA = false>
__global__ __launch_bounds__(256, 2) void ffn_fused_bwd_kernel(FfnBwdArgs q) {
  const GemmArgs& p = q.e;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int tm = xcd_remap(blockIdx.x, p.ntm);
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int nch = q.f >> 7;

  // stage copies.  A (dy2) as plane_gemm_kernel's: wave w's instruction i fills KiB 2w + i of the A image = rows
  // 16 (2w + i) .. + 15, lane j -> row + j / 4, physical chunk j % 4 = logical chunk (j % 4) ^ ((row >> 2) & 3)
  // (the rows are held, not the addresses: the kernel sits at the register cap)
  int arow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t gr = (int64_t)tm * GT + (2 * wave + i) * 16 + (lane >> 2);
    const int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    arow[i] = ir < 0 ? 0 : ir;
  }
  // u: wave w's instruction i fills KiB 4w + i = rows 32w + 8i .. + 7 (128 B each), lane j -> row + j / 8, physical
  // piece j % 8 = logical piece (j % 8) ^ ((row >> 1) & 7); rows the map does not name read row 0 (never stored)
  // (the rows are held, not the addresses: four VGPRs instead of eight at the register cap)
  int urow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t gr = (int64_t)tm * GT + 32 * wave + 8 * i + (lane >> 3);
    const int ur = p.out_rows ? p.out_rows[gr] : (int)gr;
    urow[i] = ur < 0 ? 0 : ur;
  }
  constexpr int64_t T1 = 8 * (int64_t)PG_B_BYTES;             // one W2 column tile: K = 128 = 8 units
  const char* img2 = reinterpret_cast<const char*>(q.img2) + (int64_t)(q.g2 ? g : 0) * nch * T1;
  const char* img1 = reinterpret_cast<const char*>(q.img1) + (int64_t)(q.g1 ? g : 0) * (q.f >> 4) * PG_B_BYTES;
  const int blane = 2 * wave * 1024 + 16 * lane;
  auto issue = [&](int c, int sidx, int buf) {
    char* sb = lds + buf * FF_STG;
    if (sidx < 8) {
      const char* bs = img2 + c * T1 + (int64_t)sidx * PG_B_BYTES + blane;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds(
            (const void*)(p.A + (int64_t)arow[i] * p.lda + 16 * sidx + 4 * ((lane & 3) ^ ((lane >> 4) & 3))),
            (lds_void_t*)(sb + (2 * wave + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(bs + i * 1024),
                                         (lds_void_t*)(sb + PG_A_BYTES + (2 * wave + i) * 1024), 16, 0, 0);
    } else if (sidx < 12) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(
            (const void*)(q.u + (int64_t)urow[i] * q.ldu + 128 * c + 32 * (sidx - 8) +
                          4 * ((lane & 7) ^ ((4 * i + (lane >> 4)) & 7))),
            (lds_void_t*)(sb + (4 * wave + i) * 1024), 16, 0, 0);
    } else {
      const char* bs = img1 + (int64_t)(8 * c + 2 * (sidx - 12)) * PG_B_BYTES + blane;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_global_load_lds((const void*)(bs + u * PG_B_BYTES + i * 1024),
                                           (lds_void_t*)(sb + u * 8192 + (2 * wave + i) * 1024), 16, 0, 0);
    }
  };

  const int ra = 32 * wave + li;                      // this lane's row of the tile
  const int aoff0 = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
  const int sw = (li >> 3) & 1;
  const int boff = PG_A_BYTES + li * 32 + 16 * (h ^ sw);
  const int woff0 = li * 32 + 16 * sw + 8 * h;        // W1: k 4h .. 4h+3 and 8 + 4h .. of the unit's 16
  const int usw = (li >> 1) & 7;                      // u stage: piece 2 qd + h of row ra

  // the row's dy2 bound (plane_gemm_kernel's a_rowmax form) and output row
  float abound = 0.f;
  int mrow;
  {
    const int64_t gr = (int64_t)tm * GT + ra;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    mrow = p.out_rows ? p.out_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    for (int j = 0; j < p.a_rowmax_n; ++j) abound = fmaxf(abound, p.a_rowmax[(int64_t)ir * p.a_rowmax_n + j]);
    if constexpr (MASKA) {
      abound *= p.drop_scale;                         // a bound on |dx2| in, a bound on |dy2| for the pair split
      unsigned char* kb = reinterpret_cast<unsigned char*>(lds + FB_TAB_OFF + (q.f + GT) * 4) + ra * (GT / 8) + h;
      // drop_keep(seed, site, base + c, thr) with the index product carried: (base + c) K = base K + c K (mod 2^32)
      const uint32_t base = (uint32_t)(tail_token(ir, p.tail_K, p.tail_I, p.tail_pos) * GT) + 8 * h;
      const uint32_t h0 = base * 0x9E3779B1u + p.seed, sx = q.a_site * 0x85EBCA77u;
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        uint32_t b = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          b |= (uint32_t)(fmix32((h0 + (uint32_t)(16 * kt + e) * 0x9E3779B1u) ^ sx) >= p.drop_thr) << e;
        kb[2 * kt] = (unsigned char)b;
      }
    }
  }
  // the images' column factors (1 / s_n, NaN for an image without the pair tag), once per tile
  // (through a copy of the thread id the compiler cannot see through: it otherwise keeps 4 t, which the epilogue's
  // dgamma store uses again, in two registers across the main loop — a spill at the register cap)
  float* tab = reinterpret_cast<float*>(lds + FB_TAB_OFF);
  int tt = t;
  asm volatile("" : "+v"(tt));
  for (int idx = tt; idx < q.f; idx += 256) {
    const float* cs = reinterpret_cast<const float*>(img2 + (idx >> 7) * T1 + 2 * GT * 16 * 2);
    const float bad = reinterpret_cast<const uint32_t*>(cs)[GT] == PAIR_IMAGE_TAG ? 1.f : __builtin_nanf("");
    tab[idx] = bad / cs[idx & 127];
  }
  if (tt < GT) {
    const float* cs = reinterpret_cast<const float*>(img1 + 2 * GT * 16 * 2);
    const float bad = reinterpret_cast<const uint32_t*>(cs)[GT] == PAIR_IMAGE_TAG ? 1.f : __builtin_nanf("");
    tab[q.f + tt] = bad / cs[tt];
  }
  int* rmeta = reinterpret_cast<int*>(lds + FF_META_OFF);
  if (h == 0) rmeta[ra] = mrow;
  if constexpr (MASKA) {
    // the rows' bits to memory for the W2 weight gradient (rows the map names only)
    __syncthreads();
    if (tt < GT) {
      const int kr = rmeta[tt];
      if (kr >= 0)
        *reinterpret_cast<u32x4*>(q.keep_out + (int64_t)kr * q.ldkeep) =
            *reinterpret_cast<const u32x4*>(lds + FB_TAB_OFF + (q.f + GT) * 4 + tt * (GT / 8));
    }
  }
  const float asc = pow2_scale14(abound);
  const float ainv = 1.f / asc;
  float* trw = reinterpret_cast<float*>(lds + FF_TR_OFF + wave * FF_TR_WAVE);
  // every load above is waited for here, before the first copy is in flight (as in ffn_fused_kernel)
  asm volatile("" : "+v"(abound), "+v"(mrow), "+v"(arow[0]), "+v"(arow[1]), "+v"(urow[0]), "+v"(urow[1]),
               "+v"(urow[2]), "+v"(urow[3]));

  int rb = 0;                                         // ring buffer of the stage waited for next
  issue(0, 0, 0);
  if (FF_NST == 3) issue(0, 1, 1);
  f32x16 acc2[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[a][r] = 0.f;
  float am = 0.f, bound = 0.f, hsc = 1.f, hinv = 1.f;

  for (int c = 0; c < nch; ++c) {
    // stage (c, sidx) has landed (every wave's after the barrier); the barrier also retires the reads of the buffer
    // that the next stage's copies then overwrite; returns the stage's buffer
    auto top = [&](int sidx) -> const char* {
      if (FF_NST == 2 || sidx == 12 || (sidx == 15 && c + 1 == nch)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      constexpr int AH = FF_NST - 1;                    // the stage copied now: AH ahead, into the buffer read last
      const int nb_ = rb == 0 ? FF_NST - 1 : rb - 1;
      if (sidx + AH < 16) issue(c, sidx + AH, nb_);
      else if (c + 1 < nch) issue(c + 1, sidx + AH - 16, nb_);
      const char* sb = lds + rb * FF_STG;
      rb = rb + 1 == FF_NST ? 0 : rb + 1;
      return sb;
    };
    f32x16 acc1[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[a][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      const char* sb = top(kt);
      u32x4 fb[4][2];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) fb[nb][pl] = *reinterpret_cast<const u32x4*>(sb + boff + pl * 4096 + nb * 1024);
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + (aoff0 ^ 16));   // chunk 2h + 1
      float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      if constexpr (MASKA) {
        // keep ? a * scale : 0 as (a & -bit) * scale: a signed one-bit field extract and an AND per element
        const int kb = *reinterpret_cast<const unsigned char*>(lds + FB_TAB_OFF + (q.f + GT) * 4 + ra * (GT / 8) +
                                                               2 * kt + h);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          av[e] = __uint_as_float(__float_as_uint(av[e]) & (uint32_t)((kb << (31 - e)) >> 31)) * p.drop_scale;
      }
      u32x4 fa[3];
      pair8(av, asc, fa);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc1[nb] = mfma_pair_t(fb[nb], fa, acc1[nb]);
    }
    // ---- dU of this chunk, in registers: 32 columns per u stage
    float ua = 0.f;
    auto finish = [&](int nb, f32x16& a) {
      const char* sb = top(8 + nb);
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const f32x4 u4 = *reinterpret_cast<const f32x4*>(sb + ra * 128 + 16 * ((2 * qd + h) ^ usw));
        const f32x4 ci = *reinterpret_cast<const f32x4*>(tab + 128 * c + 32 * nb + 8 * qd + 4 * h);
        f32x4 v = {a[4 * qd], a[4 * qd + 1], a[4 * qd + 2], a[4 * qd + 3]};
        v = v * (ainv * ci);
        v *= gelu_erf_grad4(u4);
        ua = amax4(ua, v);
        a[4 * qd] = v.x; a[4 * qd + 1] = v.y; a[4 * qd + 2] = v.z; a[4 * qd + 3] = v.w;
      }
    };
    finish(0, acc1[0]);
    finish(1, acc1[1]);
    finish(2, acc1[2]);
    finish(3, acc1[3]);
    if (mrow >= 0) am = fmaxf(am, ua);
    bound = fmaxf(bound, fmaxf(ua, __shfl_xor(ua, 32, 64)));
    {
      const float s = pow2_scale14(bound);
      if (c > 0) {
        const float ratio = s * hinv;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc2[a][r] *= ratio;
      }
      hsc = s;
      hinv = 1.f / s;
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        *reinterpret_cast<f32x4*>(trw + li * FF_TR_LD + 8 * qd + 4 * h) =
            f32x4{acc1[nb][4 * qd], acc1[nb][4 * qd + 1], acc1[nb][4 * qd + 2], acc1[nb][4 * qd + 3]};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's writes before its reads
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(trw + ((lane >> 3) + 8 * ps) * FF_TR_LD + 4 * (lane & 7));
        const int ur = rmeta[32 * wave + (lane >> 3) + 8 * ps];     // (published by the main loop's barriers)
        if (ur >= 0) store_out4(q.du + (int64_t)ur * q.lddu + 128 * c + 32 * nb + 4 * (lane & 7), v);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // rewritten by the next pass
    }
    // ---- GEMM2: acc1[j] is the B operand of the chunk's units 2j, 2j + 1
    auto stage2 = [&](int j, const f32x16& u) {
      const char* sb = top(12 + j);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float hv[8] = {u[8 * s], u[8 * s + 1], u[8 * s + 2], u[8 * s + 3],
                             u[8 * s + 4], u[8 * s + 5], u[8 * s + 6], u[8 * s + 7]};
        u32x4 fh[3];
        pair8(hv, hsc, fh);
        u32x4 fw[4][2];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) {
            const char* wb = sb + s * 8192 + pl * 4096 + nb * 1024;
            const u32x2 lo = *reinterpret_cast<const u32x2*>(wb + woff0);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(wb + (woff0 ^ 16));
            fw[nb][pl] = u32x4{lo.x, lo.y, hi.x, hi.y};
          }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc2[nb] = mfma_pair_t(fw[nb], fh, acc2[nb]);
      }
    };
    stage2(0, acc1[0]);
    stage2(1, acc1[1]);
    stage2(2, acc1[2]);
    stage2(3, acc1[3]);
  }
  // unscale: the last chunk's row scale (per lane), W1's column factors (per register)
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const f32x4 cs = *reinterpret_cast<const f32x4*>(tab + q.f + 32 * nb + 8 * qd + 4 * h);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc2[nb][4 * qd + i] *= hinv * cs[i];
    }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                    // the epilogue reuses the stage buffers
  gemm_vec_epilogue<EPIT, 5, false, OT_PLANE_EPI_RBN, false>(p, acc2, smem, tm, 0, g, 0, -1, rmeta);
  if (q.du_amax) amax_flush(q.du_amax, am);           // (uniform: every wave reaches it)
}

// 1 (default: measured faster, profiles/r13/ffn_fused_bwd.md) = the model's block backward takes ot_ffn_fused_bwd where
// its form applies, 0 = the FFN2 and FFN1 dgrad launches; the environment variable ONETRANS_FFN_FUSED_BWD (0 / 1) sets
// the process's initial value
#ifndef OT_FFN_FUSED_BWD
#define OT_FFN_FUSED_BWD 1
#endif
static int ffn_fused_bwd_initial() {
  const char* e = getenv("ONETRANS_FFN_FUSED_BWD");
  return e && *e ? (atoi(e) != 0) : OT_FFN_FUSED_BWD;
}
static std::atomic<int> g_ffn_fused_bwd{ffn_fused_bwd_initial()};

// 1 (default: measured faster, profiles/r15/bwd_mask_fused.md) = where the model's block backward takes
// ot_ffn_fused_bwd under dropout, the kernel masks dx2 itself (ot_ffn_fused_bwd_mask) and the W2 weight gradient masks
// from its keep bits (OT_WG_D_KEEPBITS): no dropout pass, no dy2; 0 = the dropout pass; the environment variable
// ONETRANS_BWD_MASK_FUSED (0 / 1) sets the process's initial value
#ifndef OT_BWD_MASK_FUSED
#define OT_BWD_MASK_FUSED 1
#endif
static int bwd_mask_fused_initial() {
  const char* e = getenv("ONETRANS_BWD_MASK_FUSED");
  return e && *e ? (atoi(e) != 0) : OT_BWD_MASK_FUSED;
}
static std::atomic<int> g_bwd_mask_fused{bwd_mask_fused_initial()};

}  // namespace ot

using namespace ot;

extern "C" int ot_ffn_fused_bwd_on(int on) {
  const int old = g_ffn_fused_bwd.load(std::memory_order_relaxed);
  if (on >= 0) g_ffn_fused_bwd.store(on ? 1 : 0, std::memory_order_relaxed);
  return old;
}

// ot_ffn_fused_bwd (mask false) and ot_ffn_fused_bwd_mask
static int ffn_fused_bwd_impl(const ot_ffn_fused_bwd_args* a, bool mask, uint32_t mask_site, uint32_t* keep_out,
                              int64_t ldkeep, void* stream) {
  OT_REQUIRE(a, "ot_ffn_fused_bwd: null arguments");
  OT_REQUIRE(a->struct_size == sizeof(ot_ffn_fused_bwd_args),
             "ot_ffn_fused_bwd: ot_ffn_fused_bwd_args.struct_size %zu != %zu (header of another ot_version)",
             a->struct_size, sizeof(ot_ffn_fused_bwd_args));
  OT_REQUIRE(a->dy2 && a->dy2_rowmax && a->u && a->du && a->w2_image && a->w1_image && a->x1 && a->gamma && a->rstd &&
                 a->dx1 && a->dgamma && a->workspace,
             "ot_ffn_fused_bwd: null operand");
  OT_REQUIRE(a->ntiles >= 0 && a->f >= GT && a->f % GT == 0 && a->f <= FF_MAX_F,
             "ot_ffn_fused_bwd: bad sizes ntiles=%d f=%d (f a multiple of %d up to %d)", a->ntiles, a->f, GT, FF_MAX_F);
  auto a16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  OT_REQUIRE(a->lddy2 >= GT && a->ldx1 >= GT && a->lddx1 >= GT && a->lddy2 % 4 == 0 && a->ldx1 % 4 == 0 &&
                 a->lddx1 % 4 == 0 && a16(a->dy2) && a16(a->x1) && a16(a->dx1) && a16(a->gamma) && a16(a->w2_image) &&
                 a16(a->w1_image),
             "ot_ffn_fused_bwd: rows of %d floats, leading dimensions multiples of 4, 16-B aligned operands", GT);
  OT_REQUIRE(a->ldu >= a->f && a->lddu >= a->f && a->ldu % 4 == 0 && a->lddu % 4 == 0 && a16(a->u) && a16(a->du),
             "ot_ffn_fused_bwd: u / du need ld >= f, ld %% 4 == 0 and 16-B alignment");
  OT_REQUIRE(a->dy2_rowmax_n >= 1, "ot_ffn_fused_bwd: dy2_rowmax_n must be >= 1");
  OT_REQUIRE(!a->dres || (a->lddres >= GT && a->lddres % 4 == 0 && a16(a->dres)),
             "ot_ffn_fused_bwd: dres needs lddres >= %d, lddres %% 4 == 0 and 16-B alignment", GT);
  OT_REQUIRE(a->w1_groups >= 1 && a->w2_groups >= 1, "ot_ffn_fused_bwd: image group counts must be >= 1");
  OT_REQUIRE(a->w1_groups == 1 && a->w2_groups == 1 ? true : a->tile_group != nullptr,
             "ot_ffn_fused_bwd: grouped weight images need tile_group");
  OT_REQUIRE(a->drop_rate >= 0.f && a->drop_rate < 1.f, "ot_ffn_fused_bwd: drop_rate out of range");
  OT_REQUIRE(a->drop_rate == 0.f || (a->tail_K > 0 && a->tail_I >= a->tail_K), "ot_ffn_fused_bwd: bad tail map");
  OT_REQUIRE(a->drop_rate == 0.f || (a->dx_masked && a->lddxm >= GT && a->lddxm % 4 == 0 && a16(a->dx_masked)),
             "ot_ffn_fused_bwd: dropout needs dx_masked (lddxm >= %d, lddxm %% 4 == 0, 16-B aligned)", GT);
  OT_REQUIRE(a->ws_bytes >= ot_mixed_gemm_rms_workspace_size(a->ntiles, GT), "ot_ffn_fused_bwd: workspace too small");
  OT_REQUIRE(!a->rowabs_out || a->rowabs_n == 1, "ot_ffn_fused_bwd: rowabs_out needs rowabs_n == 1");
  OT_REQUIRE(!mask || (a->drop_rate > 0.f && keep_out && ldkeep >= GT / 32 && ldkeep % 4 == 0 && a16(keep_out)),
             "ot_ffn_fused_bwd_mask: needs drop_rate > 0 and keep_out (ldkeep >= %d, ldkeep %% 4 == 0, 16-B aligned)",
             GT / 32);
  if (a->ntiles == 0) return OT_OK;
  FfnBwdArgs q{};
  GemmArgs& p = q.e;
  p.A = a->dy2; p.lda = a->lddy2; p.K = a->f; p.in_rows = a->rows;
  p.a_rowmax = a->dy2_rowmax; p.a_rowmax_n = a->dy2_rowmax_n;
  p.N = GT; p.tile_group = a->tile_group;
  p.C = a->dx1; p.ldc = a->lddx1; p.out_rows = a->rows;
  p.seed = a->seed; p.site = a->site; p.drop_thr = 0u; p.drop_scale = 1.f;
  p.tail_K = a->tail_K > 0 ? a->tail_K : 1; p.tail_I = a->tail_I > 0 ? a->tail_I : 1; p.tail_pos = a->tail_pos;
  p.drop_width = GT; p.ntm = a->ntiles; p.ntn = 1;
  p.nx = a->x1; p.ldnx = a->ldx1; p.ngamma = a->gamma; p.nrstd = a->rstd;
  p.dres = a->dres; p.lddres = a->lddres;
  p.dxm = a->dx_masked; p.lddxm = a->lddxm;
  p.dgpart = (float*)a->workspace;
  p.amax_out = a->amax_out; p.rowabs_out = a->rowabs_out; p.rowabs_n = a->rowabs_n;
  int epi = OT_EPI_RMSNORM_BWD;
  if (a->drop_rate > 0.f) {
    epi |= OT_EPI_DROPOUT;
    p.drop_thr = drop_threshold(a->drop_rate);
    p.drop_scale = 1.f / (1.f - a->drop_rate);
  }
  p.epi = epi;
  q.img2 = a->w2_image; q.g2 = a->w2_groups > 1;
  q.img1 = a->w1_image; q.g1 = a->w1_groups > 1;
  q.u = a->u; q.ldu = a->ldu; q.du = a->du; q.lddu = a->lddu; q.du_amax = a->du_amax; q.f = a->f;
  q.a_site = mask_site; q.keep_out = keep_out; q.ldkeep = ldkeep;
  void (*kern)(FfnBwdArgs) = mask                 ? ffn_fused_bwd_kernel<OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT, true>
                             : a->drop_rate > 0.f ? ffn_fused_bwd_kernel<OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT>
                                                  : ffn_fused_bwd_kernel<OT_EPI_RMSNORM_BWD>;
  static std::once_flag once;                          // more than 64 KiB of LDS: opt in
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)ffn_fused_bwd_kernel<OT_EPI_RMSNORM_BWD>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, ffn_bwd_lds(FF_MAX_F));
    (void)hipFuncSetAttribute((const void*)ffn_fused_bwd_kernel<OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, ffn_bwd_lds(FF_MAX_F));
    (void)hipFuncSetAttribute((const void*)ffn_fused_bwd_kernel<OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT, true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, ffn_bwd_lds(FF_MAX_F, true));
    (void)hipGetLastError();
  });
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kern, dim3((unsigned)a->ntiles), dim3(256), (size_t)ffn_bwd_lds(a->f, mask), s, q);
  OT_LAUNCH_CHECK("ot_ffn_fused_bwd");
  float* dgpart = (float*)a->workspace;
  launch_colsum_reduce(dgpart, a->ntiles, GT, a->dgamma, a->accumulate_dgamma, s, dgpart + (int64_t)a->ntiles * GT);
  OT_LAUNCH_CHECK("ot_ffn_fused_bwd(dgamma)");
  return OT_OK;
}

extern "C" int ot_ffn_fused_bwd(const ot_ffn_fused_bwd_args* a, void* stream) {
  return ffn_fused_bwd_impl(a, false, 0u, nullptr, 0, stream);
}

extern "C" int ot_ffn_fused_bwd_mask(const ot_ffn_fused_bwd_args* a, uint32_t mask_site, uint32_t* keep_out,
                                     int64_t ldkeep, void* stream) {
  return ffn_fused_bwd_impl(a, true, mask_site, keep_out, ldkeep, stream);
}

extern "C" int ot_bwd_mask_fused(int on) {
  const int old = g_bwd_mask_fused.load(std::memory_order_relaxed);
  if (on >= 0) g_bwd_mask_fused.store(on ? 1 : 0, std::memory_order_relaxed);
  return old;
}

extern "C" int ot_ffn_fused(int on) {
  const int old = g_ffn_fused.load(std::memory_order_relaxed);
  if (on >= 0) g_ffn_fused.store(on ? 1 : 0, std::memory_order_relaxed);
  return old;
}

extern "C" int ot_ffn_fused_fwd(const ot_ffn_fused_args* a, void* stream) {
  OT_REQUIRE(a, "ot_ffn_fused_fwd: null arguments");
  OT_REQUIRE(a->struct_size == sizeof(ot_ffn_fused_args),
             "ot_ffn_fused_fwd: ot_ffn_fused_args.struct_size %zu != %zu (header of another ot_version)",
             a->struct_size, sizeof(ot_ffn_fused_args));
  OT_REQUIRE(a->x1 && a->x2 && a->rstd && a->w1_image && a->w2_image && a->b1 && a->b2,
             "ot_ffn_fused_fwd: null operand");
  OT_REQUIRE(a->ntiles >= 0 && a->f >= GT && a->f % GT == 0 && a->f <= FF_MAX_F,
             "ot_ffn_fused_fwd: bad sizes ntiles=%d f=%d (f a multiple of %d up to %d)", a->ntiles, a->f, GT, FF_MAX_F);
  auto a16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  OT_REQUIRE(a->ldx1 >= GT && a->ldx2 >= GT && a->ldx1 % 4 == 0 && a->ldx2 % 4 == 0 && a16(a->x1) && a16(a->x2) &&
                 a16(a->b1) && a16(a->b2) && a->b1_gstride % 4 == 0 && a->b2_gstride % 4 == 0 && a16(a->w1_image) &&
                 a16(a->w2_image),
             "ot_ffn_fused_fwd: rows of %d floats, leading dimensions and bias strides multiples of 4, 16-B aligned "
             "operands", GT);
  OT_REQUIRE(!a->u_out || (a->ldu >= a->f && a->ldu % 4 == 0 && a16(a->u_out)),
             "ot_ffn_fused_fwd: u_out needs ldu >= f, ldu %% 4 == 0 and 16-B alignment");
  OT_REQUIRE(a->w1_groups >= 1 && a->w2_groups >= 1, "ot_ffn_fused_fwd: image group counts must be >= 1");
  OT_REQUIRE(a->w1_groups == 1 && a->w2_groups == 1 ? true : a->tile_group != nullptr,
             "ot_ffn_fused_fwd: grouped weight images need tile_group");
  OT_REQUIRE(a->drop_rate >= 0.f && a->drop_rate < 1.f, "ot_ffn_fused_fwd: drop_rate out of range");
  OT_REQUIRE(a->drop_rate == 0.f || (a->tail_K > 0 && a->tail_I >= a->tail_K), "ot_ffn_fused_fwd: bad tail map");
  if (a->ntiles == 0) return OT_OK;
  FfnArgs q{};
  GemmArgs& p = q.e;
  p.A = a->x1; p.lda = a->ldx1; p.K = GT; p.in_rows = a->rows; p.a_xform = OT_AX_RMSNORM; p.a_rstd = a->rstd;
  p.N = GT; p.tile_group = a->tile_group; p.bias = a->b2; p.bias_gstride = a->b2_gstride;
  p.C = a->x2; p.ldc = a->ldx2; p.out_rows = a->rows;
  p.res = a->x1; p.ldres = a->ldx1; p.res_tok = 0;
  p.seed = a->seed; p.site = a->site; p.drop_thr = 0u; p.drop_scale = 1.f;
  p.tail_K = a->tail_K > 0 ? a->tail_K : 1; p.tail_I = a->tail_I > 0 ? a->tail_I : 1; p.tail_pos = a->tail_pos;
  p.drop_width = GT; p.ntm = a->ntiles; p.ntn = 1;
  p.rstd_out = a->rstd_out; p.eps = a->eps;
  int epi = OT_EPI_BIAS | OT_EPI_RESIDUAL;
  if (a->drop_rate > 0.f) {
    epi |= OT_EPI_DROPOUT;
    p.drop_thr = drop_threshold(a->drop_rate);
    p.drop_scale = 1.f / (1.f - a->drop_rate);
  }
  if (a->rstd_out) epi |= OT_EPI_ROW_RSTD;
  p.epi = epi;
  q.img1 = a->w1_image; q.g1 = a->w1_groups > 1;
  q.img2 = a->w2_image; q.g2 = a->w2_groups > 1;
  q.b1 = a->b1; q.b1_gstride = a->b1_gstride;
  q.u_out = a->u_out; q.ldu = a->ldu; q.u_amax = a->u_amax; q.f = a->f;
  void (*kern)(FfnArgs) = nullptr;
#define OT_FFN_PICK(EP_) if (epi == (EP_)) kern = ffn_fused_kernel<EP_>;
  OT_FFN_PICK(OT_EPI_BIAS | OT_EPI_RESIDUAL)
  OT_FFN_PICK(OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT)
  OT_FFN_PICK(OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)
  OT_FFN_PICK(OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)
#undef OT_FFN_PICK
  static std::once_flag once;                          // more than 64 KiB of LDS: opt in
  std::call_once(once, [] {
#define OT_FFN_ATTR(EP_)                                                                                            \
  (void)hipFuncSetAttribute((const void*)ffn_fused_kernel<EP_>, hipFuncAttributeMaxDynamicSharedMemorySize,         \
                            ffn_lds(FF_MAX_F));
    OT_FFN_ATTR(OT_EPI_BIAS | OT_EPI_RESIDUAL)
    OT_FFN_ATTR(OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT)
    OT_FFN_ATTR(OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)
    OT_FFN_ATTR(OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)
#undef OT_FFN_ATTR
    (void)hipGetLastError();
  });
  hipLaunchKernelGGL(kern, dim3((unsigned)a->ntiles), dim3(256), (size_t)ffn_lds(a->f), (hipStream_t)stream, q);
  OT_LAUNCH_CHECK("ot_ffn_fused_fwd");
  return OT_OK;
}
