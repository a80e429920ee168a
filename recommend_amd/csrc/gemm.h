// What more than one of the GEMM files needs: the tile constants, GemmArgs, the vector epilogue, the plane
// images' stage sizes and the per-family kernel pick functions that mixed_gemm_impl (gemm.hip) dispatches through.
//   gemm.hip             mixed_gemm_impl and the ot_mixed_gemm* exports, row_rstd_finish_kernel, mixed_gemm_kernel's
//                        edge-tile forms
//   gemm_mixed.h / .hip  mixed_gemm_kernel / its whole-tile forms
//   gemm_plane.hip       plane_gemm_kernel, plane_panel_kernel
//   gemm_plane_wide.hip  plane_wide_kernel, plane_big_kernel, plane_sq_kernel
//   gemm_images.hip      the pre-split weight images (ot_split_images)
//   gemm_wgrad.hip       the weight-gradient kernels, their reduce and the transposed weight shadow
// Every kernel instantiation is compiled in exactly one of these files.
#pragma once
#include "common.h"

namespace ot {

#ifndef OT_GEMM_BK
#define OT_GEMM_BK 16
#endif
#ifndef OT_PLANE_EPI_RBN          // epilogue rows per operand-load batch of the 4-workgroup plane GEMMs
#define OT_PLANE_EPI_RBN 4
#endif
constexpr int GT = 128;           // tile rows / cols
constexpr int GBK = OT_GEMM_BK;   // k per LDS stage (16 or 32)
constexpr int GLD = GBK + 4;      // LDS row stride (floats)

// Split-bf16 MFMA (OT_GEMM_SPLIT = number of product terms, 0 = native f32 MFMA).  Every f32
// operand is split exactly into three bf16 pieces x = x0 + x1 + x2 (x0 = top 8 significant bits,
// x1 the next 8, x2 the last 8; truncation keeps every step exact), and a.b = sum_ij ai.bj with
// each bf16 x bf16 product exact in the f32 accumulator of v_mfma_f32_32x32x16_bf16 (32 cycles per
// 32x32x16 against 64 cycles per 32x32x2 for the f32 form: 16x the rate).  9 terms = every
// product (the f32 result up to accumulation order); 6 terms drop a1.b2, a2.b1, a2.b2, whose sum
// is below 2^-22 |a||b| — the size of one f32 rounding of the product.
#ifndef OT_GEMM_SPLIT
#define OT_GEMM_SPLIT 6           // product terms of the split kernels (6 or 9; 3 is not f32-accurate)
#endif
#ifndef OT_GEMM_NT_STORE
#define OT_GEMM_NT_STORE 1        // epilogue output rows written with non-temporal (streaming) stores
                                  // (C2 +0.5%, T +0.5%: profiles/r02/gemm_nt_store.txt); 0: plain stores
#endif
constexpr int SPLIT_TERMS = OT_GEMM_SPLIT;
static_assert(SPLIT_TERMS == 3 || SPLIT_TERMS == 6 || SPLIT_TERMS == 9, "OT_GEMM_SPLIT");
static_assert(GBK == 16, "split-bf16 staging assumes 16-k stages");

struct GemmArgs {
  const float* A; int64_t lda; int K;
  const int32_t* in_rows;                       // [ntm*GT] or null (identity)
  int a_xform; const float* a_rstd; const float* a_gamma;
  const float* W; int64_t w_gstride; int64_t ldw; int N;
  const int32_t* tile_group;                    // [ntm] or null (group 0)
  const float* bias; int64_t bias_gstride;
  float* C; int64_t ldc; const int32_t* out_rows;
  int epi;
  const float* res; int64_t ldres; int res_tok;
  const float* aux; int64_t ldaux;
  uint32_t seed, site, drop_thr; float drop_scale; int tail_K, tail_I; int drop_width;
  int ntm, ntn;
  // row-norm epilogues (N == GT: the tile holds whole rows; OT_EPI_ROW_RSTD also N > GT on the plane
  // GEMM: per-tile row sums of squares in rowpart, finished by row_rstd_finish_kernel)
  float* rstd_out; float eps;                                   // OT_EPI_ROW_RSTD
  const float* nx; int64_t ldnx; const float* ngamma; const float* nrstd;   // OT_EPI_RMSNORM_BWD
  const float* dres; int64_t lddres; int dres_K, dres_I; const int32_t* dres_inv;
  float* dxm; int64_t lddxm; float* dgpart;
  float* rowpart;                               // OT_EPI_ROW_RSTD with N > GT: [ntm*GT][ntn] row sums of squares
  float* rowdot; int rowdot_n;                  // OT_EPI_ROWDOT output / OT_EPI_RMSNORM_BWD (N > GT) input
  uint16_t* gelu_out; int64_t ldgelu;           // bf16 gelu_erf(aux) with OT_EPI_GELU_BWD, bf16 gelu_erf(C) with
                                                // epi == OT_EPI_BIAS (optional)
  const int32_t* tail_pos;                      // kept positions (ot_pyramid_select) or null (tail)
  // plane GEMM: pre-split B image (ot_split_images), its tiles per group and the first tile used
  const uint16_t* bimg; int bimg_ntn, bimg_tn0;
  // plane GEMM with the RMSNorm prologue: the first column tile's workgroups also store bf16(a * gamma * rstd)
  // of their A rows (the bf16 weight gradient's normalised A operand)
  uint16_t* xn_out; int64_t ldxn;
  uint16_t* c16_out; int64_t ldc16;             // bf16-mode plane GEMM: also C rounded to bf16 (optional)
  float* rowmax_out; int rowmax_n;              // split plane GEMM: per (out row, column tile) max of C after bias
  const float* a_rowmax; int a_rowmax_n;        // split plane GEMM, GELU prologue: A's row maxima (pair arithmetic)
  float* amax_out;                              // vector epilogue: atomic max of |stored output| (pair wgrad bound)
  float* rowabs_out; int rowabs_n;              // vector epilogue: per (out row, column tile) max |stored output|
  int rowmeta;                                  // pair plane GEMM: row metadata parked in LDS (ot_plane_rowmeta)
  int panel_w;                                  // panel plane GEMM: column tiles per workgroup
};

// sum over the 32 lanes that hold one output row in the vector epilogue (same order as the
// row-wise kernels' group_sum with 32 threads per row)
// max over the 32 lanes that hold one output row (the vector epilogue's row maxima): within each 16-lane row by
// DPP (quad swaps, half-row and row mirrors), then across the two rows by v_permlane16_swap — VALU only, where
// five __shfl_xor steps were five ds_bpermute LDS round trips per row (max is order-free: the same result)
__device__ __forceinline__ float row32_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));   // quad [1,0,3,2]
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));   // quad [2,3,0,1]
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));  // row_half_mirror
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));  // row_mirror
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
__device__ __forceinline__ float row32_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- vector epilogue shared by the GEMM kernels (compile-time flags EPIT >= 0, no edge tiles): the
// accumulator tile goes through LDS (the staging buffers are free: the caller's last barrier ended
// every main-loop read) in two 64-row halves; each thread then finishes 8 rows x one float4 column
// chunk, so every global access is a 16-B piece of a 512-B row run and each row index is loaded once
// per row instead of once per element.  Operand loads of a batch of rows are issued together.
// LAYOUT 0: 2x2 waves, acc[2m + n] = rows 64 (wave >> 1) + 32 m, cols 64 (wave & 1) + 32 n;
// LAYOUT 1: 4x1 waves, acc[nb] = rows 32 wave, cols 32 nb; LAYOUT 2 (a 128-column half `sub` of a 256-column
// tile held by 2x2 waves): wave 2 r + sub holds rows 64 r + 32 m, cols 32 nb in acc[4 m + nb]; LAYOUT 3 (128-column
// quarter `sub` of a 512-column tile): wave `sub` holds all 128 rows, rows 32 m / cols 32 nb in acc[4 m + nb];
// LAYOUT 4 (128-column half `sub` of a 256 x 256 tile's row half, the epilogue run by that row half's four waves
// with thread ids `tid` 0..255): wave 2 sub + j holds all 128 rows x columns 64 j + 32 nb in acc[2 m + nb];
// LAYOUT 5 (4x1 waves, transposed accumulators: the fused FFN, gemm_ffn.hip): lane li holds row 32 wave + li,
// acc[nb][r] = column 32 nb + (r & 3) + 8 (r >> 2) + 4 h.
// ROWSCALE: multiply row r by
// a_rstd[in_rows[r]] first (the plane GEMM's RMSNorm prologue, folded into the weights).
__device__ __forceinline__ void store_out4(float* dst, f32x4 v) {
  if (OT_GEMM_NT_STORE) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst));
  else *reinterpret_cast<f32x4*>(dst) = v;
}
// four values rounded to bf16 (8 B), streamed like store_out4: the bf16-mode outputs (C, gelu(U), the bf16
// residual copies) are the bulk of those GEMMs' traffic, and written through the L2 they evict the A rows the
// tile's neighbours in N still read
#ifndef OT_GEMM_NT_STORE16
#define OT_GEMM_NT_STORE16 1
#endif
__device__ __forceinline__ void store_out4_bf16(uint16_t* dst, f32x4 v) {
  if (OT_GEMM_NT_STORE16) __builtin_nontemporal_store(bf16_rne4(v), reinterpret_cast<u32x2*>(dst));
  else *reinterpret_cast<u32x2*>(dst) = bf16_rne4(v);
}

// GS: compile the forward stored-GELU path (bf16-mode plane GEMM only: registers elsewhere)
// rmeta (pair plane GEMM, LAYOUT 1): the tile's 128 output rows and, with ROWSCALE, its 128 row factors (float
// bits) behind them, parked in LDS by the kernel's prologue — the same values the global row maps give, read
// without the per-row load -> wait -> dependent load chain (null: read the row maps here).
template <int EPIT, int LAYOUT, bool ROWSCALE, int RBN = 8, bool GS = false>
__device__ __forceinline__ void gemm_vec_epilogue(const GemmArgs& p, const f32x16* acc, float* smem, int tm,
                                                  int n0, int g, int sub = 0, int tid = -1,
                                                  const int* rmeta = nullptr) {
  const int epi = EPIT;
  const int t = tid >= 0 ? tid : (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
    // ---- vector epilogue: the accumulator tile goes through LDS (the staging buffers are free: the
    // last main-loop barrier ended every read) in two 64-row halves; each thread then finishes 8
    // rows x one float4 column chunk, so every global access is a 16-B piece of a 512-B row run and
    // each row index is loaded once per row instead of once per element.  Operand loads of a batch
    // of rows are issued together.
    constexpr int CLD = GT + 4;
    static_assert(64 * CLD + 8 * GT <= 4 * GT * GLD, "epilogue LDS exceeds the staging buffers");
    float* ct = smem;                                   // [64][CLD]
    const int c4 = t & 31, rb = t >> 5;                 // float4 column chunk, first local row
    const int col = n0 + 4 * c4;
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (epi & OT_EPI_BIAS) bias4 = *reinterpret_cast<const f32x4*>(p.bias + (int64_t)g * p.bias_gstride + col);
    const bool need_tok = (epi & OT_EPI_DROPOUT) || ((epi & OT_EPI_RESIDUAL) && p.res_tok);
    constexpr bool RMSBWD = EPIT >= 0 && (EPIT & OT_EPI_RMSNORM_BWD);
    constexpr bool ROWRSTD = EPIT >= 0 && (EPIT & OT_EPI_ROW_RSTD);
    constexpr bool ROWDOT = EPIT >= 0 && (EPIT & OT_EPI_ROWDOT);
    // gelu_out of a bias-only epilogue: gelu(C) (C in f32 or bf16)
    constexpr bool GSTORE = GS && (EPIT == OT_EPI_BIAS || EPIT == (OT_EPI_BIAS | OT_EPI_C_BF16));
    constexpr bool CBF = EPIT >= 0 && (EPIT & OT_EPI_C_BF16);
    constexpr bool AUXBF = EPIT >= 0 && (EPIT & OT_EPI_AUX_BF16);
    f32x4 rdb4 = {0.f, 0.f, 0.f, 0.f};                 // OT_EPI_ROWDOT: the bias subtracted from aux
    if (ROWDOT) rdb4 = *reinterpret_cast<const f32x4*>(p.bias + (int64_t)g * p.bias_gstride + col);
    // dgamma partials live in a thread-private LDS slot behind ct (a register accumulator here
    // costs the whole kernel ~70 VGPRs of occupancy): dgs[rb][4 c4 .. 4 c4 + 3]
    float* dgs = ct + 64 * CLD;
    f32x4 ngam = {0.f, 0.f, 0.f, 0.f};
    if (RMSBWD) {
      ngam = *reinterpret_cast<const f32x4*>(p.ngamma + col);
      *reinterpret_cast<f32x4*>(dgs + rb * GT + 4 * c4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    constexpr int RB = RMSBWD ? RBN / 2 : RBN;          // rows per operand-load batch (register budget)
    float am = 0.f;                                     // amax_out: |the output the next consumer reads|
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      // this half's output rows (the loads stay in flight across the accumulator write below)
      int orow[8];
      float rsc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int lr = rb + 8 * i;                      // local row of the half: tile row below
        const int64_t gr = (int64_t)tm * GT + (LAYOUT == 0 ? (lr >> 5) * 64 + 32 * hf + (lr & 31) : 64 * hf + lr);
        if ((LAYOUT == 1 || LAYOUT == 5) && rmeta) {    // parked by the kernel's prologue
          orow[i] = rmeta[64 * hf + lr];
          if (ROWSCALE) rsc[i] = __int_as_float(rmeta[GT + 64 * hf + lr]);
          continue;
        }
        orow[i] = p.out_rows ? p.out_rows[gr] : (int)gr;
        if (ROWSCALE) {                                 // RMSNorm folded into B: scale by the A row's rstd
          const int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
          rsc[i] = ir >= 0 ? p.a_rstd[ir] : 0.f;
        }
      }
      if (LAYOUT == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            ct[((wave >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * CLD + (wave & 1) * 64 + 32 * n + li] = acc[2 * hf + n][r];
      } else if (LAYOUT == 1) {
        if ((wave >> 1) == hf) {
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              ct[((wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * CLD + 32 * nb + li] = acc[nb][r];
        }
      } else if (LAYOUT == 5) {                         // LAYOUT 5: lane = row, four consecutive columns per store
        if ((wave >> 1) == hf) {
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
              *reinterpret_cast<f32x4*>(ct + ((wave & 1) * 32 + li) * CLD + 32 * nb + 8 * qd + 4 * h) =
                  f32x4{acc[nb][4 * qd], acc[nb][4 * qd + 1], acc[nb][4 * qd + 2], acc[nb][4 * qd + 3]};
        }
      } else if (LAYOUT == 4) {                         // LAYOUT 4: waves 2 sub, 2 sub + 1 (64 columns each)
        if ((wave >> 1) == sub) {
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
              for (int r = 0; r < 16; ++r)
                ct[(32 * m + (r & 3) + 8 * (r >> 2) + 4 * h) * CLD + 64 * (wave & 1) + 32 * nb + li] =
                    acc[2 * (2 * hf + m) + nb][r];
        }
      } else if (LAYOUT == 3) {                         // LAYOUT 3: sub-tile `sub` is wave `sub`'s 16 blocks
        if (wave == sub) {
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
              for (int r = 0; r < 16; ++r)
                ct[(32 * m + (r & 3) + 8 * (r >> 2) + 4 * h) * CLD + 32 * nb + li] = acc[4 * (2 * hf + m) + nb][r];
        }
      } else if ((wave >> 1) == hf && (wave & 1) == sub) {   // LAYOUT 2: this half's rows are one wave's 64
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              ct[(32 * m + (r & 3) + 8 * (r >> 2) + 4 * h) * CLD + 32 * nb + li] = acc[4 * m + nb][r];
      }
      __syncthreads();
#pragma unroll
      for (int i0 = 0; i0 < 8; i0 += RB) {
        int64_t tok[RB];
        f32x4 aux4[RB], res4[RB], cp4[RB], x4[RB], dr4[RB];
        float nr[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int orr = orow[i0 + i];
          const int64_t o = orr < 0 ? 0 : orr;
          tok[i] = (need_tok && orr >= 0) ? tail_token(orr, p.tail_K, p.tail_I, p.tail_pos) : o;
          if (RMSBWD) {
            x4[i] = *reinterpret_cast<const f32x4*>(p.nx + o * p.ldnx + col);
            nr[i] = p.nrstd[o];
            dr4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p.dres) {
              const int64_t dr = p.dres_K > 0 ? kept_row(o, p.dres_K, p.dres_I, p.dres_inv) : o;
              if (dr >= 0) dr4[i] = *reinterpret_cast<const f32x4*>(p.dres + (int64_t)dr * p.lddres + col);
            }
          }
          if (AUXBF) {
            const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.aux) + o * p.ldaux + col);
            aux4[i] = f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                            __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
          } else if (epi & OT_EPI_GELU_BWD) {
            aux4[i] = *reinterpret_cast<const f32x4*>(p.aux + o * p.ldaux + col);
          }
          if (epi & OT_EPI_RESIDUAL)
            res4[i] = *reinterpret_cast<const f32x4*>(p.res + (p.res_tok ? tok[i] : o) * p.ldres + col);
          if (epi & OT_EPI_ACCUMULATE) cp4[i] = *reinterpret_cast<const f32x4*>(p.C + o * p.ldc + col);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int orr = orow[i0 + i];
          f32x4 v = *reinterpret_cast<const f32x4*>(ct + (rb + 8 * (i0 + i)) * CLD + 4 * c4);
          if (ROWSCALE) v = v * rsc[i0 + i];
          if (epi & OT_EPI_BIAS) v += bias4;
          if (p.rowmax_out) {                                  // this tile's largest C of the row (signed)
            float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
            mx = row32_max(mx);
            if (orr >= 0 && c4 == 0) p.rowmax_out[(int64_t)orr * p.rowmax_n + n0 / GT] = mx;
          }
          if (epi & OT_EPI_GELU_BWD) {
            v *= gelu_erf_grad4(aux4[i]);
            if (p.gelu_out && orr >= 0) {                      // the stored GELU (W2 weight gradient's A)
              const f32x4 hv = gelu_erf4(aux4[i]);
              store_out4_bf16(p.gelu_out + (int64_t)orr * p.ldgelu + col, hv);
            }
            if (ROWDOT) {                                      // this tile's part of sum_f dU_f (U_f - b_f)
              const f32x4 ub = aux4[i] - rdb4;
              const float sd = row32_sum(v.x * ub.x + v.y * ub.y + v.z * ub.z + v.w * ub.w);
              if (orr >= 0 && c4 == 0) p.rowdot[(int64_t)orr * p.rowdot_n + n0 / GT] = sd;
            }
          }
          if (epi & OT_EPI_GELU) {
            v = gelu_erf4(v);
          }
          if (RMSBWD) {
            // v = dL/dy of y = x * rstd * gamma:  dx = rstd * (g - x * rstd^2 * <g, x> / N) + dres
            const f32x4 gv = v * ngam;
            const float r = nr[i];
            float sdot;
            if (p.rowdot) {                                    // N > GT: <g dy, x> = sum of the partials / rstd
              float t = 0.f;
              const float* rp = p.rowdot + (int64_t)(orr < 0 ? 0 : orr) * p.rowdot_n;
              for (int j = 0; j < p.rowdot_n; ++j) t += rp[j];
              sdot = t / r;
            } else {
              sdot = row32_sum(gv.x * x4[i].x + gv.y * x4[i].y + gv.z * x4[i].z + gv.w * x4[i].w);
            }
            const float coef = r * r * r * sdot / (float)p.N;
            if (orr >= 0) {
              f32x4* q = reinterpret_cast<f32x4*>(dgs + rb * GT + 4 * c4);
              *q = *q + v * x4[i] * r;
            }
            v = gv * r - x4[i] * coef + dr4[i];
            if (orr >= 0) store_out4(p.C + (int64_t)orr * p.ldc + col, v);
            if (!(epi & OT_EPI_DROPOUT) && orr >= 0) am = amax4(am, v);
            f32x4 cv = v;                                      // what the next consumer reads (mask(dx) or dx)
            if ((epi & OT_EPI_DROPOUT) && orr >= 0) {          // mask(dx) for the dropout site upstream
              const uint32_t idx = (uint32_t)(tok[i] * p.drop_width + col);
              f32x4 mv;
              mv.x = drop_keep(p.seed, p.site, idx + 0, p.drop_thr) ? v.x * p.drop_scale : 0.f;
              mv.y = drop_keep(p.seed, p.site, idx + 1, p.drop_thr) ? v.y * p.drop_scale : 0.f;
              mv.z = drop_keep(p.seed, p.site, idx + 2, p.drop_thr) ? v.z * p.drop_scale : 0.f;
              mv.w = drop_keep(p.seed, p.site, idx + 3, p.drop_thr) ? v.w * p.drop_scale : 0.f;
              store_out4(p.dxm + (int64_t)orr * p.lddxm + col, mv);
              am = amax4(am, mv);
              cv = mv;
            }
            if (p.rowabs_out) {                                // the consumer's row bound (dx_masked, else dx)
              float mx = amax4(0.f, cv);
              mx = row32_max(mx);
              if (orr >= 0 && c4 == 0) p.rowabs_out[(int64_t)orr * p.rowabs_n + n0 / GT] = mx;
            }
            continue;
          }
          if (epi & OT_EPI_DROPOUT) {
            const uint32_t idx = (uint32_t)(tok[i] * p.drop_width + col);
            v.x = drop_keep(p.seed, p.site, idx + 0, p.drop_thr) ? v.x * p.drop_scale : 0.f;
            v.y = drop_keep(p.seed, p.site, idx + 1, p.drop_thr) ? v.y * p.drop_scale : 0.f;
            v.z = drop_keep(p.seed, p.site, idx + 2, p.drop_thr) ? v.z * p.drop_scale : 0.f;
            v.w = drop_keep(p.seed, p.site, idx + 3, p.drop_thr) ? v.w * p.drop_scale : 0.f;
          }
          if (epi & OT_EPI_RESIDUAL) v += res4[i];
          if (epi & OT_EPI_ACCUMULATE) v += cp4[i];
          if (ROWRSTD) {                                       // rstd of the finished row (next RMSNorm)
            const float ss = row32_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
            if (p.rowpart) {                                   // N > GT: this tile's part of the row sum
              if (c4 == 0) {
                const int lr = rb + 8 * (i0 + i);
                const int64_t gr = (int64_t)tm * GT + (LAYOUT == 0 ? (lr >> 5) * 64 + 32 * hf + (lr & 31) : 64 * hf + lr);
                p.rowpart[gr * p.ntn + n0 / GT] = ss;
              }
            } else if (orr >= 0 && c4 == 0) {
              p.rstd_out[orr] = rsqrtf(ss / (float)p.N + p.eps);
            }
          }
          if (GSTORE && p.gelu_out && orr >= 0) {              // FFN1 forward: also gelu(U) in bf16
            const f32x4 hv = gelu_erf4(v);
            store_out4_bf16(p.gelu_out + (int64_t)orr * p.ldgelu + col, hv);
          }
          if (GS && p.c16_out && orr >= 0)                     // + a bf16 copy of C (the next GEMM's A)
            store_out4_bf16(p.c16_out + (int64_t)orr * p.ldc16 + col, v);
          if (CBF) {                                           // C in bf16 (the FFN2 dgrad's dU)
            if (orr >= 0) store_out4_bf16(reinterpret_cast<uint16_t*>(p.C) + (int64_t)orr * p.ldc + col, v);
          } else if (orr >= 0) {
            store_out4(p.C + (int64_t)orr * p.ldc + col, v);
          }
          if (orr >= 0) am = amax4(am, v);
          if (p.rowabs_out) {                                  // this tile's max |C| of the row (fp16-pair consumer)
            float mx = amax4(0.f, v);
            mx = row32_max(mx);
            if (orr >= 0 && c4 == 0) p.rowabs_out[(int64_t)orr * p.rowabs_n + n0 / GT] = mx;
          }
        }
      }
      __syncthreads();                                  // ct is rewritten by the next half
    }
    if (RMSBWD && t < GT) {                             // dgamma partial of this tile (fixed order)
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) a += dgs[k * GT + t];
      p.dgpart[(int64_t)tm * p.N + n0 + t] = a;
    }
    if (p.amax_out) amax_flush(p.amax_out, am);          // (uniform: every wave reaches it)
}

// ---- plane images (ot_split_images, gemm_images.hip) as the plane GEMMs (gemm_plane.hip, gemm_plane_wide.hip)
// copy them: one 16-k stage of a 128-column tile
constexpr int PG_B_BYTES = 3 * GT * 16 * 2;        // B stage image: 3 planes x 128 n x 16 bf16

typedef __attribute__((address_space(3))) void lds_void_t;

// Pair-form images carry a tag behind their 128 column scales (plane 2 of the tile's first unit, float 128): the
// TERMS-2 plane GEMM refuses (all-NaN output) an image without it, and the tag's bytes are two bf16 quiet NaNs, so a
// six-product kernel handed a pair image multiplies NaN into its outputs (plane 2 at n = 16, k = 0, 1) instead of
// silently reading the scales as a third bf16 plane.  (The C ABI cannot see an image's form: the host layer pairs
// the images with a_rowmax, recommend_amd/model.py; this makes a mismatch loud.)
constexpr uint32_t PAIR_IMAGE_TAG = 0x7FC17FC1u;

// ---- the kernel of each family for (a_xform, epi), or null where the family has no such specialisation; the
// dynamic LDS bytes that form's stages need come back through the pointer.  Each function lives with its kernels
// and opts them in to more than 64 KiB of LDS where they need it.
// mixed_gemm_kernel's whole-tile forms (gemm_mixed.hip; the edge-tile forms are with the dispatch).  splt: 0 native
// f32 MFMA, 1 OT_MATMUL_BF16, SPLIT_TERMS split-bf16.  _generic: the run-time prologue / epilogue kernel, never null
void (*mixed_gemm_whole_for(bool nt, int x, int e, int splt))(GemmArgs);
void (*mixed_gemm_whole_generic(bool nt, int splt))(GemmArgs);
// plane_gemm_kernel (gemm_plane.hip).  one: OT_MATMUL_BF16; rowmax: the caller gave A's row maxima (pair arithmetic)
void (*plane_gemm_for(int x, int e, bool one, bool rowmax, int* stage_lds))(GemmArgs);
// plane_panel_kernel (gemm_plane.hip).  variant 0: three workgroups per CU; 1: four; 2: two, A fragments held
void (*plane_panel_for(int x, int e, int variant, int* lds))(GemmArgs);
int plane_panel_width(int ntiles, int ntn);        // column tiles per workgroup (0: stay on plane_gemm_kernel)
void plane_panel_launched();                       // counts a launch for ot_plane_panel_launches
// gemm_plane_wide.hip.  kind 1: 128 x 256 (plane_wide_kernel), 2: 128 x 512 (plane_big_kernel), 3: 256 x 256
// (plane_sq_kernel)
void (*plane_wide_for(int x, int e, int kind, int* stage_lds))(GemmArgs);
int plane_tile_auto(int K, int N, int ntiles);     // the kind ot_plane_wide(1) takes for a shape (0: 128 x 128)
constexpr int PW_COLS = 2 * GT;                    // columns of a kind 1 / 3 tile
constexpr int PB_COLS = 4 * GT;                    // columns of a kind 2 tile

}  // namespace ot
