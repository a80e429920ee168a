// mixed_gemm_kernel, the register-staged GEMM, and the pick of its instantiations.  Two files instantiate it, one
// EDGE value each (compile time: together they are as much device code as every plane GEMM): gemm.hip the edge-tile
// forms (EDGE = true), gemm_mixed.hip the whole-tile forms (EDGE = false).
#pragma once
#include <algorithm>
#include <mutex>

#include "gemm.h"

namespace ot {

#ifndef OT_GEMM_MINWG
#define OT_GEMM_MINWG 3
#endif
#ifndef OT_GEMM_PRIO
#define OT_GEMM_PRIO 0
#endif
#ifndef OT_GEMM_RMS_EARLY
#define OT_GEMM_RMS_EARLY 1
#endif
#ifndef OT_GEMM_SPLIT_SCHED
#define OT_GEMM_SPLIT_SCHED 0     // >0: interleave this many VALU ops after each MFMA (sched_group_barrier)
#endif
constexpr int SRS = 3 * 16 + 8;   // split LDS row stride (ushorts): 3 planes x 16 k + pad = 112 B
// SPLT template argument of the split kernels: 0 = native f32 MFMA, SPLIT_TERMS = split-bf16,
// 1 = OT_MATMUL_BF16 (one bf16 plane rounded to nearest: bf16 MFMA on f32 data, f32 accumulation)

// AXT / EPIT: compile-time prologue / epilogue (-1 = read p.a_xform / p.epi at run time).
// EDGE: K % 32 != 0 or N % 128 != 0 (bounds checks in staging and epilogue).
// SPLT: split-bf16 MFMA (NT only; the main loop's LDS images and register sets limit it to 2
// workgroups per CU), else native f32 MFMA.
template <bool NT, int AXT, int EPIT, bool EDGE, int SPLT>
__global__ __launch_bounds__(256, (NT && SPLT) ? 2 : OT_GEMM_MINWG) void mixed_gemm_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                      // [2][GT][GLD]
  float* Bs = smem + 2 * GT * GLD;       // [2][GT][GLD]
  const int ax = AXT >= 0 ? AXT : p.a_xform;
  const int epi = EPIT >= 0 ? EPIT : p.epi;
  constexpr bool SPL = NT && SPLT != 0;
  constexpr int TERMS = SPLT;

  const int nwg = p.ntm * p.ntn;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / p.ntn, tn = wg % p.ntn;
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const float* W = p.W + (int64_t)g * p.w_gstride;
  const int n0 = tn * GT;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  // ---- staging coordinates: a row holds CPR float4 chunks; thread t stages chunk sc of rows
  // sr + RPP*i (i < NPASS), for A and (NT) B
  // (Consecutive lanes read consecutive 16-B chunks of a row.  Remapping the 8 lanes of each
  // ds_write_b128 group onto 8 rows makes the stores conflict-free but costs ~8 % on the loads.)
  constexpr int CPR = GBK / 4, RPP = 256 / CPR, NPASS = GT / RPP;
  const int sc = t % CPR, sr = t / CPR;
  const float* arow[NPASS];
  const float* brow[NPASS];
  float ars[NPASS];
  bool aok[NPASS], bok[NPASS];
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    const int r = sr + RPP * i;
    const int64_t gr = (int64_t)tm * GT + r;
    const int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    aok[i] = ir >= 0;
    arow[i] = p.A + (int64_t)(ir < 0 ? 0 : ir) * p.lda + 4 * sc;
    ars[i] = (ax == OT_AX_RMSNORM && ir >= 0) ? p.a_rstd[ir] : 1.f;
    const int n = n0 + r;
    bok[i] = !EDGE || n < p.N;
    brow[i] = W + (int64_t)(bok[i] ? n : 0) * p.ldw + 4 * sc;
  }
  // load_stage issues raw, branch-free loads (invalid rows / k read a clamped in-bounds address and
  // are zeroed at store time); the prologue transform runs in store_stage, after the MFMA block, so
  // the global loads of stage k+1 stay in flight across the MFMAs of stage k.
  // (measured: the cheap RMSNorm scale is best applied right at load time, GELU at store time)
  constexpr bool RMS_EARLY = OT_GEMM_RMS_EARLY;
  f32x4 ra[NPASS], rb[NPASS], gm;
  bool kin = true;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // NN B staging: lane reads W[k0 + kk][n0 + 4*n4 ...], kk = lane % GBK
  const int nn_kk = lane % GBK, nn_n4 = wave * (64 / GBK) + lane / GBK;
  bool nnok[NPASS];

  auto load_stage = [&](int k0) {
    kin = !EDGE || (k0 + 4 * sc < p.K);
    const int ko = kin ? k0 : -4 * sc;                       // clamped: column 0 of the row
    if (ax == OT_AX_RMSNORM) gm = *reinterpret_cast<const f32x4*>(p.a_gamma + ko + 4 * sc);
#pragma unroll
    for (int i = 0; i < NPASS; ++i) ra[i] = *reinterpret_cast<const f32x4*>(arow[i] + ko);
    if (RMS_EARLY && ax == OT_AX_RMSNORM) {
#pragma unroll
      for (int i = 0; i < NPASS; ++i) ra[i] = ra[i] * gm * ars[i];
    }
    if (NT) {
#pragma unroll
      for (int i = 0; i < NPASS; ++i) rb[i] = *reinterpret_cast<const f32x4*>(brow[i] + ko);
    } else {
#pragma unroll
      for (int i = 0; i < NPASS; ++i) {
        const int k = k0 + nn_kk, n = n0 + 4 * (nn_n4 + (256 / GBK) * i);
        nnok[i] = !EDGE || (k < p.K && n < p.N);
        rb[i] = *reinterpret_cast<const f32x4*>(W + (nnok[i] ? (int64_t)k * p.ldw + n : 0));
      }
    }
  };
  auto store_stage = [&](int buf) {
    float* as = As + buf * GT * GLD;
    float* bs = Bs + buf * GT * GLD;
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      f32x4 v = ra[i];
      if (!RMS_EARLY && ax == OT_AX_RMSNORM) {
        v = v * gm * ars[i];
      } else if (ax == OT_AX_GELU) {
        v = gelu_erf4(v);
      }
      if (!(aok[i] && kin)) v = zero4;
      *reinterpret_cast<f32x4*>(as + (sr + RPP * i) * GLD + 4 * sc) = v;
    }
    if (NT) {
#pragma unroll
      for (int i = 0; i < NPASS; ++i)
        *reinterpret_cast<f32x4*>(bs + (sr + RPP * i) * GLD + 4 * sc) = (bok[i] && kin) ? rb[i] : zero4;
    } else {
#pragma unroll
      for (int i = 0; i < NPASS; ++i) {
        const int n = 4 * (nn_n4 + (256 / GBK) * i);
        const f32x4 v = nnok[i] ? rb[i] : zero4;
        bs[(n + 0) * GLD + nn_kk] = v.x;
        bs[(n + 1) * GLD + nn_kk] = v.y;
        bs[(n + 2) * GLD + nn_kk] = v.z;
        bs[(n + 3) * GLD + nn_kk] = v.w;
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nk = (p.K + GBK - 1) / GBK;
  if constexpr (SPL) {
    // ---- split-bf16 main loop.  A 16-k stage is 4x fewer MFMA cycles than in f32, so the global
    // loads run two stages ahead (two register sets, loop unrolled by 2): stage k+2 is issued before
    // the MFMAs of stage k, stage k+1 (issued one iteration earlier) is split into LDS after them.
    struct SStage { f32x4 a[NPASS], b[NPASS], g; bool kin; };
    auto sload = [&](SStage& st, int k0) {
      st.kin = !EDGE || (k0 + 4 * sc < p.K);
      const int ko = st.kin ? k0 : -4 * sc;
      if (ax == OT_AX_RMSNORM) st.g = *reinterpret_cast<const f32x4*>(p.a_gamma + ko + 4 * sc);
#pragma unroll
      for (int i = 0; i < NPASS; ++i) st.a[i] = *reinterpret_cast<const f32x4*>(arow[i] + ko);
      if (RMS_EARLY && ax == OT_AX_RMSNORM) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i) st.a[i] = st.a[i] * st.g * ars[i];
      }
#pragma unroll
      for (int i = 0; i < NPASS; ++i) st.b[i] = *reinterpret_cast<const f32x4*>(brow[i] + ko);
    };
    // split images [row][plane][16 k] (ushorts, row stride SRS = 112 B): a lane's 8-k read of one
    // plane is a 16-B piece, and 16 consecutive rows land in 16 distinct bank groups
    struct SPlanes { u32x2 a[NPASS][3], b[NPASS][3]; };
    auto ssplit = [&](const SStage& st, SPlanes& q) {
#pragma unroll
      for (int i = 0; i < NPASS; ++i) {
        f32x4 v = st.a[i];
        if (!RMS_EARLY && ax == OT_AX_RMSNORM) {
          v = v * st.g * ars[i];
        } else if (ax == OT_AX_GELU) {
          v = gelu_erf4(v);
        }
        if (!(aok[i] && st.kin)) v = zero4;
        const f32x4 w = (bok[i] && st.kin) ? st.b[i] : zero4;
        if constexpr (TERMS == 1) {
          q.a[i][0] = bf16_rne4(v);
          q.b[i][0] = bf16_rne4(w);
        } else {
          split3(v, q.a[i][0], q.a[i][1], q.a[i][2]);
          split3(w, q.b[i][0], q.b[i][1], q.b[i][2]);
        }
      }
    };
    auto swrite = [&](const SPlanes& q, int buf) {
      uint16_t* as16 = reinterpret_cast<uint16_t*>(smem) + buf * GT * SRS;
      uint16_t* bs16 = reinterpret_cast<uint16_t*>(smem) + (2 + buf) * GT * SRS;
#pragma unroll
      for (int i = 0; i < NPASS; ++i)
#pragma unroll
        for (int pl = 0; pl < (TERMS == 1 ? 1 : 3); ++pl) {
          *reinterpret_cast<u32x2*>(as16 + (sr + RPP * i) * SRS + 16 * pl + 4 * sc) = q.a[i][pl];
          *reinterpret_cast<u32x2*>(bs16 + (sr + RPP * i) * SRS + 16 * pl + 4 * sc) = q.b[i][pl];
        }
    };
    auto smma = [&](int buf) {
      const uint16_t* as16 = reinterpret_cast<const uint16_t*>(smem) + buf * GT * SRS + (wm + li) * SRS + 8 * h;
      const uint16_t* bs16 = reinterpret_cast<const uint16_t*>(smem) + (2 + buf) * GT * SRS + (wn + li) * SRS + 8 * h;
      u32x4 fa[2][3], fb[2][3];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < (TERMS == 1 ? 1 : 3); ++q) {
          fa[m][q] = *reinterpret_cast<const u32x4*>(as16 + 32 * m * SRS + 16 * q);
          fb[m][q] = *reinterpret_cast<const u32x4*>(bs16 + 32 * m * SRS + 16 * q);
        }
      // smallest terms first; (plane of A, plane of B)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if constexpr (TERMS == 1) {
            acc[m][n] = mfma_bf16(fa[m][0], fb[n][0], acc[m][n]);
            continue;
          }
          if (SPLIT_TERMS >= 9) {
            acc[m][n] = mfma_bf16(fa[m][2], fb[n][2], acc[m][n]);
            acc[m][n] = mfma_bf16(fa[m][1], fb[n][2], acc[m][n]);
            acc[m][n] = mfma_bf16(fa[m][2], fb[n][1], acc[m][n]);
          }
          if (SPLIT_TERMS >= 6) {
            acc[m][n] = mfma_bf16(fa[m][0], fb[n][2], acc[m][n]);
            acc[m][n] = mfma_bf16(fa[m][2], fb[n][0], acc[m][n]);
            acc[m][n] = mfma_bf16(fa[m][1], fb[n][1], acc[m][n]);
          }
          acc[m][n] = mfma_bf16(fa[m][0], fb[n][1], acc[m][n]);
          acc[m][n] = mfma_bf16(fa[m][1], fb[n][0], acc[m][n]);
          acc[m][n] = mfma_bf16(fa[m][0], fb[n][0], acc[m][n]);
        }
    };
    // one stage: issue the loads two stages ahead, MFMAs of the LDS stage interleaved with the split
    // of the next stage (already in registers), which is then written to the other buffer.
    // Branch-free (the loads past the end re-read the last stage; the extra image is never read)
    // so the whole stage is one scheduling region.
    auto stage = [&](SStage& ld, const SStage& nx, int kload, int buf) {
      sload(ld, kload);
      SPlanes q;
      ssplit(nx, q);
      smma(buf);
      swrite(q, buf ^ 1);
#if OT_GEMM_SPLIT_SCHED
#pragma unroll
      for (int i = 0; i < 4 * SPLIT_TERMS; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, OT_GEMM_SPLIT_SCHED, 0);
      }
#endif
      __syncthreads();
    };
    SStage s0, s1;
    sload(s0, 0);
    sload(s1, nk > 1 ? GBK : 0);
    {
      SPlanes q;
      ssplit(s0, q);
      swrite(q, 0);
    }
    __syncthreads();
    const int klast = (nk - 1) * GBK;
    for (int kt = 0; kt < nk; kt += 2) {
      stage(s0, s1, min((kt + 2) * GBK, klast), 0);     // stage kt in buf 0, kt+1 in s1
      if (kt + 1 >= nk) break;
      stage(s1, s0, min((kt + 3) * GBK, klast), 1);     // stage kt+1 in buf 1, kt+2 in s0
    }
  } else {
  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load_stage((kt + 1) * GBK);
    const float* as = As + cur * GT * GLD + (wm + li) * GLD + (GBK / 2) * h;
    const float* bs = Bs + cur * GT * GLD + (wn + li) * GLD + (GBK / 2) * h;
#pragma unroll
    for (int half = 0; half < GBK / 16; ++half) {
      f32x4 fa[2][2], fb[2][2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          fa[m][q] = *reinterpret_cast<const f32x4*>(as + 32 * m * GLD + 8 * half + 4 * q);
          fb[m][q] = *reinterpret_cast<const f32x4*>(bs + 32 * m * GLD + 8 * half + 4 * q);
        }
      if (OT_GEMM_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[m][s >> 2][s & 3], fb[n][s >> 2][s & 3],
                                                             acc[m][n], 0, 0, 0);
      if (OT_GEMM_PRIO) __builtin_amdgcn_s_setprio(0);
    }
    // the other buffer was last read in iteration kt-1, which every wave finished before the
    // barrier that ended it: one barrier per k-tile
    if (more) store_stage(cur ^ 1);
    __syncthreads();
  }
  }

  // ---- epilogue (flags compile-time unless EPIT < 0).  Per 32-row block m: resolve the 16 output
  // rows of this lane, issue every operand load (aux / residual / accumulate source) for the block,
  // then compute and store — no load-use chains per element.
  if constexpr (!EDGE && EPIT >= 0) {
    const f32x16 acc4[4] = {acc[0][0], acc[0][1], acc[1][0], acc[1][1]};
    gemm_vec_epilogue<EPIT, 0, false>(p, acc4, smem, tm, n0, g);
    return;
  }
  // ---- scalar epilogue (EDGE: N % 128 != 0 or unaligned operands; generic run-time flags)
  float bias_v[2] = {0.f, 0.f};
  int cols[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    cols[n] = n0 + wn + 32 * n + li;
    if ((epi & OT_EPI_BIAS) && (!EDGE || cols[n] < p.N)) bias_v[n] = p.bias[(int64_t)g * p.bias_gstride + cols[n]];
  }
  const bool need_tok = (epi & OT_EPI_DROPOUT) || ((epi & OT_EPI_RESIDUAL) && p.res_tok);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    int orow[16];
    int64_t tok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      const int64_t gr = (int64_t)tm * GT + row;
      orow[r] = p.out_rows ? p.out_rows[gr] : (int)gr;
      tok[r] = (need_tok && orow[r] >= 0) ? tail_token(orow[r], p.tail_K, p.tail_I, p.tail_pos) : orow[r];
    }
    float ld0[16][2];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        float v = 0.f;
        const bool ok = orow[r] >= 0 && (!EDGE || cols[n] < p.N);
        if (ok) {
          if (epi & OT_EPI_GELU_BWD) v = p.aux[(int64_t)orow[r] * p.ldaux + cols[n]];
          else if (epi & OT_EPI_RESIDUAL) v = p.res[(p.res_tok ? tok[r] : (int64_t)orow[r]) * p.ldres + cols[n]];
          else if (epi & OT_EPI_ACCUMULATE) v = p.C[(int64_t)orow[r] * p.ldc + cols[n]];
        }
        ld0[r][n] = v;
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (orow[r] < 0) continue;
      float* crow = p.C + (int64_t)orow[r] * p.ldc;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = cols[n];
        if (EDGE && col >= p.N) continue;
        float v = acc[m][n][r];
        if (epi & OT_EPI_BIAS) v += bias_v[n];
        if (epi & OT_EPI_GELU_BWD) v *= gelu_erf_grad(ld0[r][n]);
        if (epi & OT_EPI_GELU) v = gelu_erf(v);
        if (epi & OT_EPI_DROPOUT) {
          const uint32_t idx = (uint32_t)(tok[r] * p.drop_width + col);
          v = drop_keep(p.seed, p.site, idx, p.drop_thr) ? v * p.drop_scale : 0.f;
        }
        if (epi & OT_EPI_RESIDUAL) {
          if (!(epi & OT_EPI_GELU_BWD)) v += ld0[r][n];
          else v += p.res[(p.res_tok ? tok[r] : (int64_t)orow[r]) * p.ldres + col];
        }
        if (epi & OT_EPI_ACCUMULATE) {
          if (!(epi & (OT_EPI_GELU_BWD | OT_EPI_RESIDUAL))) v += ld0[r][n];
          else v += crow[col];
        }
        crow[col] = v;
      }
    }
  }
}

// the (a_xform, epi) pairs mixed_gemm_kernel is specialised for (NT mode; every other call runs the generic kernel)
#define OT_MIXED_LIST(X)                                                                       \
  X(OT_AX_RMSNORM, 0)                                                                          \
  X(OT_AX_RMSNORM, OT_EPI_BIAS)                                                                \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT)                                \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL)                                                 \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_DROPOUT)                                              \
  X(OT_AX_NONE, OT_EPI_RESIDUAL)                                                               \
  X(OT_AX_NONE, OT_EPI_BIAS)                                                                   \
  X(OT_AX_NONE, OT_EPI_GELU_BWD)                                                               \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_ROWDOT)                                               \
  X(OT_AX_NONE, 0)                                                                             \
  X(OT_AX_NONE, OT_EPI_ACCUMULATE)                                                             \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)                            \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                                             \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)              \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                               \
  X(OT_AX_NONE, OT_EPI_RMSNORM_BWD)                                                            \
  X(OT_AX_NONE, OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT)

// splt: 0 native f32 MFMA, 1 OT_MATMUL_BF16, anything else SPLIT_TERMS (split-bf16); both NT only beyond 0
#define OT_MIXED_KERNEL(NT_, AX_, EP_)                                                         \
  (splt == 1 ? mixed_gemm_kernel<NT_, AX_, EP_, EDGE, 1>                                        \
   : splt    ? mixed_gemm_kernel<NT_, AX_, EP_, EDGE, SPLIT_TERMS> : mixed_gemm_kernel<NT_, AX_, EP_, EDGE, 0>)

// the specialised mixed_gemm_kernel<.., EDGE, ..> for (a_xform, epi), or null.  (Instantiates them: call it with
// the EDGE value of the calling file only.)
template <bool EDGE>
void (*mixed_gemm_pick(bool nt, int x, int e, int splt))(GemmArgs) {
#define OT_MIXED_PICK(AX_, EP_) \
  if (nt && x == (AX_) && e == (EP_)) return OT_MIXED_KERNEL(true, AX_, EP_);
  OT_MIXED_LIST(OT_MIXED_PICK)
#undef OT_MIXED_PICK
  return nullptr;
}

// any other combination: the generic instantiation (run-time prologue / epilogue)
template <bool EDGE>
void (*mixed_gemm_pick_generic(bool nt, int splt))(GemmArgs) {
  static std::once_flag lds_once;   // opt every instantiation in to > 64 KiB LDS (gfx950: 160 KiB per CU)
  std::call_once(lds_once, [] {
    const int bytes = (int)std::max(4 * GT * GLD * sizeof(float), 4 * GT * SRS * sizeof(uint16_t));
    for (void (*k)(GemmArgs) : {mixed_gemm_kernel<true, -1, -1, EDGE, 0>, mixed_gemm_kernel<false, -1, -1, EDGE, 0>,
                                mixed_gemm_kernel<true, -1, -1, EDGE, SPLIT_TERMS>,
                                mixed_gemm_kernel<true, -1, -1, EDGE, 1>})
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    (void)hipGetLastError();
  });
  if (nt) return OT_MIXED_KERNEL(true, -1, -1);
  return mixed_gemm_kernel<false, -1, -1, EDGE, 0>;
}
#undef OT_MIXED_KERNEL
#undef OT_MIXED_LIST

}  // namespace ot
