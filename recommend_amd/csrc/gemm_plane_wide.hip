// The bf16-mode plane GEMM on wider tiles (dispatch: mixed_gemm_impl, gemm.hip): plane_wide_kernel (128 x 256),
// plane_big_kernel (128 x 512) and plane_sq_kernel (256 x 256), with the ot_plane_wide switch.
#include <atomic>
#include <mutex>

#include "gemm.h"

namespace ot {

// Wide plane GEMM (OT_MATMUL_BF16, N % 256 == 0, K % 32 == 0): the plane GEMM's bf16 form on tiles of 128 rows x
// 256 columns with 32 k per stage.  A 128 x 128 tile moves 512 B through L2 -> LDS per 32x32x16 MFMA and 4 MFMAs per
// wave sit between two barriers; at C5's sizes (M = 530k rows, K 512-2048) that tile ran at 12-26% of the bf16 MFMA
// rate with its L2 -> CU stream far below what L2 serves.  Here one A fragment feeds 8 MFMAs (each wave: rows 32 w,
// all 256 columns), a stage is 384 B per MFMA and 16 MFMAs per wave sit between barriers.  A stage is two 16-k
// sub-stages in the plane GEMM's own LDS images (A as there; B = plane 0 of the two 128-column image blocks), copied
// by global_load_lds; three stages for bf16 A (72 KiB, two workgroups per CU), two for f32 A.  The epilogue is the
// plane GEMM's, once per 128-column half (same outputs, bit for bit: one MFMA chain per output in the same k order).
#ifndef OT_PLANE_WIDE
#define OT_PLANE_WIDE 1
#endif
#ifndef OT_PLANE_WIDE_WL
#define OT_PLANE_WIDE_WL 2
#endif
template <int AXT>
constexpr bool pw_abf() { return AXT == OT_AX_BF16 || AXT == OT_AX_BF16_RMSNORM; }
template <int AXT>
constexpr int pw_abytes() { return pw_abf<AXT>() ? GT * 32 : GT * 64; }      // one 16-k A image
template <int AXT>
constexpr int pw_sub() { return pw_abytes<AXT>() + 2 * GT * 32; }            // + B plane 0 of two column blocks
template <int AXT>
constexpr int pw_nstg() { return pw_abf<AXT>() ? 3 : 2; }
template <int AXT>
constexpr int pw_stage_lds() { return pw_nstg<AXT>() * 2 * pw_sub<AXT>(); }

template <int AXT, int EPIT, int WL = OT_PLANE_WIDE_WL>
__global__ __launch_bounds__(256, 2) void plane_wide_kernel(GemmArgs p) {
  static_assert(AXT == OT_AX_NONE || pw_abf<AXT>(), "wide plane GEMM: A in f32 (rounded) or bf16");
  constexpr bool ABF = pw_abf<AXT>();
  constexpr bool RSC = AXT == OT_AX_BF16_RMSNORM;
  constexpr int NSTG = pw_nstg<AXT>();
  constexpr int ABYTES = pw_abytes<AXT>();
  constexpr int SUB = pw_sub<AXT>();
  constexpr int STG = 2 * SUB;
  constexpr int OPS = 2 * ((ABF ? 1 : 2) + 2);        // copies per wave and stage
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int ntw = p.N / PW_COLS;
  const int nwg = p.ntm * ntw;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / ntw, tw = wg % ntw;
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const int n0 = tw * PW_COLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int nk = p.K >> 4, ns = nk >> 1;

  // A copy sources as in plane_gemm_kernel (rows of the tile past the row map read row 0: never stored)
  const float* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (2 * wave + i) * 16 + (lane >> 2);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrc[i] = p.A + (int64_t)ir * p.lda + 4 * ((lane & 3) ^ ((r >> 2) & 3));
  }
  const char* asrcb;
  {
    const int r = 32 * wave + (lane >> 1);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrcb = reinterpret_cast<const char*>(p.A) + ((int64_t)ir * p.lda + 8 * ((lane & 1) ^ ((r >> 3) & 1))) * 2;
  }
  const int gb = p.w_gstride ? g : 0;
  const char* bsrc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
    bsrc[c] = reinterpret_cast<const char*>(p.bimg) +
              ((int64_t)gb * p.bimg_ntn + p.bimg_tn0 + 2 * tw + c) * nk * PG_B_BYTES + wave * 1024 + 16 * lane;

  auto issue = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ks = 2 * s + j;
      char* sb = lds + buf * STG + j * SUB;
      if (ABF) {
        __builtin_amdgcn_global_load_lds((const void*)(asrcb + 32 * ks), (lds_void_t*)(sb + wave * 1024), 16, 0, 0);
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + 16 * ks), (lds_void_t*)(sb + (2 * wave + i) * 1024),
                                           16, 0, 0);
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
        __builtin_amdgcn_global_load_lds((const void*)(bsrc[c] + (int64_t)ks * PG_B_BYTES),
                                         (lds_void_t*)(sb + ABYTES + c * 4096 + wave * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  // WL 1: wave w = rows 32 w, all 256 columns (acc[c * 4 + nb]); WL 2: wave 2 r + c = rows 64 r + 32 m, columns
  // 128 c + 32 nb (acc[4 m + nb]): 6 fragment reads per 8 MFMAs instead of 9
  constexpr int NA = WL == 2 ? 2 : 1;                 // A fragments per 16-k step
  const int wr = WL == 2 ? wave >> 1 : wave, wc = WL == 2 ? wave & 1 : 0;
  int aoff0[NA], aoff1[NA], aoffb[NA];
#pragma unroll
  for (int m = 0; m < NA; ++m) {
    const int ra = (WL == 2 ? 64 : 32) * wr + 32 * m + li;
    aoff0[m] = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
    aoff1[m] = ra * 64 + 16 * ((2 * h + 1) ^ ((li >> 2) & 3));
    aoffb[m] = ra * 32 + 16 * (h ^ ((li >> 3) & 1));
  }
  const int boff = ABYTES + li * 32 + 16 * (h ^ ((li >> 3) & 1)) + wc * 4096;

  // normalised-A side output (OT_AX_BF16_RMSNORM, first column tile), as in plane_gemm_kernel (WL 2: the c = 0 waves)
  bool xnw[NA] = {};
  float xrs[NA] = {};
  uint16_t* xnp[NA] = {};
  float* gsm = reinterpret_cast<float*>(lds + NSTG * STG);
  if (RSC && p.xn_out && tw == 0) {
    for (int k = 4 * t; k < p.K; k += 4 * 256)
      *reinterpret_cast<f32x4*>(gsm + k) = *reinterpret_cast<const f32x4*>(p.a_gamma + k);
#pragma unroll
    for (int m = 0; m < NA; ++m) {
      const int64_t xgr = (int64_t)tm * GT + (WL == 2 ? 64 : 32) * wr + 32 * m + li;
      const int xir = p.in_rows ? p.in_rows[xgr] : (int)xgr;
      xnw[m] = xir >= 0 && wc == 0;
      if (xnw[m]) {
        xrs[m] = p.a_rstd[xir];
        xnp[m] = p.xn_out + (int64_t)xir * p.ldxn + 8 * h;
      }
    }
  }

  issue(0, 0);
  if (NSTG >= 3 && ns > 1) issue(1, 1);
  for (int s = 0; s < ns; ++s) {
    // this wave's copies of stage s are done (with three stages those of stage s + 1 may still fly), every
    // wave's after the barrier, which also retires the reads of the buffer the next issue overwrites
    if (NSTG >= 3 && s + 1 < ns) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(OPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s + NSTG - 1 < ns) issue(s + NSTG - 1, (s + NSTG - 1) % NSTG);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ks = 2 * s + j;
      const char* sb = lds + (s % NSTG) * STG + j * SUB;
      constexpr int NB = WL == 2 ? 4 : 8;
      u32x4 fb[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) fb[n] = *reinterpret_cast<const u32x4*>(sb + boff + (n >> 2) * 4096 + (n & 3) * 1024);
      u32x4 fa[NA];
#pragma unroll
      for (int m = 0; m < NA; ++m) {
        if constexpr (ABF) {
          fa[m] = *reinterpret_cast<const u32x4*>(sb + aoffb[m]);
          if (RSC && xnw[m]) {                          // (x * gamma) * rstd from the bf16 x, rounded
            const float* gp = gsm + 16 * ks + 8 * h;
            const u32x4 w = fa[m];
            const f32x4 a0 = {__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                              __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
            const f32x4 a1 = {__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u),
                              __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
            const u32x2 b0 = bf16_rne4(a0 * *reinterpret_cast<const f32x4*>(gp) * xrs[m]);
            const u32x2 b1 = bf16_rne4(a1 * *reinterpret_cast<const f32x4*>(gp + 4) * xrs[m]);
            *reinterpret_cast<u32x4*>(xnp[m] + 16 * ks) = u32x4{b0.x, b0.y, b1.x, b1.y};
          }
        } else {
          const f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0[m]);
          const f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + aoff1[m]);
          const u32x2 b0 = bf16_rne4(a0), b1 = bf16_rne4(a1);
          fa[m] = u32x4{b0.x, b0.y, b1.x, b1.y};
        }
      }
#pragma unroll
      for (int m = 0; m < NA; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m * NB + n] = mfma_bf16(fa[m], fb[n], acc[m * NB + n]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                    // the epilogue reuses the stage buffers
  if constexpr (WL == 2) {
    gemm_vec_epilogue<EPIT, 2, RSC, OT_PLANE_EPI_RBN, true>(p, acc, smem, tm, n0, g, 0);
    __syncthreads();                                  // (the first half's dgamma / row reads of its LDS are done)
    gemm_vec_epilogue<EPIT, 2, RSC, OT_PLANE_EPI_RBN, true>(p, acc, smem, tm, n0 + GT, g, 1);
  } else {
    gemm_vec_epilogue<EPIT, 1, RSC, OT_PLANE_EPI_RBN, true>(p, acc, smem, tm, n0, g);
    __syncthreads();
    gemm_vec_epilogue<EPIT, 1, RSC, OT_PLANE_EPI_RBN, true>(p, acc + 4, smem, tm, n0 + GT, g);
  }
}
// Big plane GEMM (OT_MATMUL_BF16, N % 512 == 0, K % 32 == 0): tiles of 128 rows x 512 columns, one workgroup of
// four waves per CU, each wave one 128 x 128 quarter (16 accumulator blocks: one A fragment feeds 4 MFMAs and one B
// fragment 4, 0.5 LDS reads per MFMA), 32 k per stage, three stages in flight (bf16 A: 120 KiB of LDS).  The
// epilogue is the plane GEMM's, once per quarter (the quarter's wave stages it through LDS).
constexpr int PB_NSTG = 3;
template <int AXT>
constexpr int pb_sub() { return pw_abytes<AXT>() + 4 * GT * 32; }            // A + B plane 0 of four column blocks
template <int AXT>
constexpr int pb_stage_lds() { return PB_NSTG * 2 * pb_sub<AXT>(); }

template <int AXT, int EPIT>
__global__ __launch_bounds__(256, 1) void plane_big_kernel(GemmArgs p) {
  static_assert(AXT == OT_AX_NONE || pw_abf<AXT>(), "big plane GEMM: A in f32 (rounded) or bf16");
  constexpr bool ABF = pw_abf<AXT>();
  constexpr bool RSC = AXT == OT_AX_BF16_RMSNORM;
  constexpr int NSTG = PB_NSTG;
  constexpr int ABYTES = pw_abytes<AXT>();
  constexpr int SUB = pb_sub<AXT>();
  constexpr int STG = 2 * SUB;
  constexpr int OPS = 2 * ((ABF ? 1 : 2) + 4);        // copies per wave and stage
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int ntw = p.N / PB_COLS;
  const int nwg = p.ntm * ntw;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / ntw, tw = wg % ntw;
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const int n0 = tw * PB_COLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int nk = p.K >> 4, ns = nk >> 1;

  const float* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (2 * wave + i) * 16 + (lane >> 2);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrc[i] = p.A + (int64_t)ir * p.lda + 4 * ((lane & 3) ^ ((r >> 2) & 3));
  }
  const char* asrcb;
  {
    const int r = 32 * wave + (lane >> 1);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrcb = reinterpret_cast<const char*>(p.A) + ((int64_t)ir * p.lda + 8 * ((lane & 1) ^ ((r >> 3) & 1))) * 2;
  }
  const int gb = p.w_gstride ? g : 0;
  const char* bsrc = reinterpret_cast<const char*>(p.bimg) +
                     ((int64_t)gb * p.bimg_ntn + p.bimg_tn0 + 4 * tw) * nk * PG_B_BYTES + wave * 1024 + 16 * lane;
  const int64_t bstride = (int64_t)nk * PG_B_BYTES;   // next 128-column image block

  auto issue = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ks = 2 * s + j;
      char* sb = lds + buf * STG + j * SUB;
      if (ABF) {
        __builtin_amdgcn_global_load_lds((const void*)(asrcb + 32 * ks), (lds_void_t*)(sb + wave * 1024), 16, 0, 0);
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + 16 * ks), (lds_void_t*)(sb + (2 * wave + i) * 1024),
                                           16, 0, 0);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
        __builtin_amdgcn_global_load_lds((const void*)(bsrc + c * bstride + (int64_t)ks * PG_B_BYTES),
                                         (lds_void_t*)(sb + ABYTES + c * 4096 + wave * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[16];
#pragma unroll
  for (int a = 0; a < 16; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  int aoff0[4], aoff1[4], aoffb[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int ra = 32 * m + li;
    aoff0[m] = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
    aoff1[m] = ra * 64 + 16 * ((2 * h + 1) ^ ((li >> 2) & 3));
    aoffb[m] = ra * 32 + 16 * (h ^ ((li >> 3) & 1));
  }
  const int boff = ABYTES + wave * 4096 + li * 32 + 16 * (h ^ ((li >> 3) & 1));

  // normalised-A side output (OT_AX_BF16_RMSNORM, first column tile): wave 0 writes every row
  bool xnw[4] = {};
  float xrs[4] = {};
  uint16_t* xnp[4] = {};
  float* gsm = reinterpret_cast<float*>(lds + NSTG * STG);
  if (RSC && p.xn_out && tw == 0) {
    for (int k = 4 * t; k < p.K; k += 4 * 256)
      *reinterpret_cast<f32x4*>(gsm + k) = *reinterpret_cast<const f32x4*>(p.a_gamma + k);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t xgr = (int64_t)tm * GT + 32 * m + li;
      const int xir = p.in_rows ? p.in_rows[xgr] : (int)xgr;
      xnw[m] = xir >= 0 && wave == 0;
      if (xnw[m]) {
        xrs[m] = p.a_rstd[xir];
        xnp[m] = p.xn_out + (int64_t)xir * p.ldxn + 8 * h;
      }
    }
  }

  issue(0, 0);
  if (ns > 1) issue(1, 1);
  for (int s = 0; s < ns; ++s) {
    if (s + 1 < ns) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(OPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s + NSTG - 1 < ns) issue(s + NSTG - 1, (s + NSTG - 1) % NSTG);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ks = 2 * s + j;
      const char* sb = lds + (s % NSTG) * STG + j * SUB;
      u32x4 fb[4], fa[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) fb[n] = *reinterpret_cast<const u32x4*>(sb + boff + n * 1024);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if constexpr (ABF) {
          fa[m] = *reinterpret_cast<const u32x4*>(sb + aoffb[m]);
          if (RSC && xnw[m]) {
            const float* gp = gsm + 16 * ks + 8 * h;
            const u32x4 w = fa[m];
            const f32x4 a0 = {__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                              __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
            const f32x4 a1 = {__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u),
                              __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
            const u32x2 b0 = bf16_rne4(a0 * *reinterpret_cast<const f32x4*>(gp) * xrs[m]);
            const u32x2 b1 = bf16_rne4(a1 * *reinterpret_cast<const f32x4*>(gp + 4) * xrs[m]);
            *reinterpret_cast<u32x4*>(xnp[m] + 16 * ks) = u32x4{b0.x, b0.y, b1.x, b1.y};
          }
        } else {
          const f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0[m]);
          const f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + aoff1[m]);
          const u32x2 b0 = bf16_rne4(a0), b1 = bf16_rne4(a1);
          fa[m] = u32x4{b0.x, b0.y, b1.x, b1.y};
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[4 * m + n] = mfma_bf16(fa[m], fb[n], acc[4 * m + n]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                    // the epilogue reuses the stage buffers
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q) __syncthreads();
    gemm_vec_epilogue<EPIT, 3, RSC, OT_PLANE_EPI_RBN, true>(p, acc, smem, tm, n0 + GT * q, g, q);
  }
}
// Square plane GEMM (OT_MATMUL_BF16, N % 256 == 0, K % 32 == 0, an even number of row tiles): 256 x 256 tiles, one
// workgroup of 8 waves per CU (2 per SIMD), wave (rh, cq) = rows 128 rh .. + 127 x columns 64 cq .. + 63 (8 blocks:
// 6 fragment reads per 8 MFMAs), 256 B of L2 -> LDS per MFMA (the 128 x 256 tile: 384; at C5's sizes that stream,
// not the MFMA, set the pace).  The tile's two 128-row halves may belong to different weight groups (tile_group):
// then each half's B image is copied into its own LDS region (uniform tiles copy one).  Epilogue: the plane GEMM's,
// each row half's four waves finishing its two 128-column quarters, both halves at once in separate LDS.
template <int AXT>
constexpr int ps_abytes() { return pw_abf<AXT>() ? 2 * GT * 32 : 2 * GT * 64; }   // one 16-k A image, 256 rows
template <int AXT>
constexpr int ps_sub() { return ps_abytes<AXT>() + 2 * (2 * GT * 32); }           // + two 256-column B planes
template <int AXT>
constexpr int ps_nstg() { return pw_abf<AXT>() ? 3 : 2; }
template <int AXT>
constexpr int ps_stage_lds() { return ps_nstg<AXT>() * 2 * ps_sub<AXT>(); }

template <int AXT, int EPIT>
__global__ __launch_bounds__(512, 1) void plane_sq_kernel(GemmArgs p) {
  static_assert(AXT == OT_AX_NONE || pw_abf<AXT>(), "square plane GEMM: A in f32 (rounded) or bf16");
  constexpr bool ABF = pw_abf<AXT>();
  constexpr bool RSC = AXT == OT_AX_BF16_RMSNORM;
  constexpr int NSTG = ps_nstg<AXT>();
  constexpr int ABYTES = ps_abytes<AXT>();
  constexpr int SUB = ps_sub<AXT>();
  constexpr int STG = 2 * SUB;
  constexpr int AOPS = ABF ? 1 : 2;                   // A copies per wave and sub-stage
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int ntw = p.N / PW_COLS;
  const int ntp = p.ntm >> 1;                          // row-tile pairs
  const int wg = xcd_remap(blockIdx.x, ntp * ntw);
  const int tp = wg / ntw, tw = wg % ntw;
  const int gA = p.tile_group ? p.tile_group[2 * tp] : 0, gB = p.tile_group ? p.tile_group[2 * tp + 1] : 0;
  const bool uni = gA == gB || p.w_gstride == 0;
  const int n0 = tw * PW_COLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int rh = wave >> 2, cq = wave & 3;
  const int nk = p.K >> 4, ns = nk >> 1;

  // A copies: bf16 A, wave w = rows 32 w .. + 31 of the 256; f32 A, instruction i of wave w = rows 16 (2 w + i) ..
  const float* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (2 * wave + i) * 16 + (lane >> 2);
    const int64_t gr = (int64_t)tp * 2 * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrc[i] = p.A + (int64_t)ir * p.lda + 4 * ((lane & 3) ^ ((r >> 2) & 3));
  }
  const char* asrcb;
  {
    const int r = 32 * wave + (lane >> 1);
    const int64_t gr = (int64_t)tp * 2 * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrcb = reinterpret_cast<const char*>(p.A) + ((int64_t)ir * p.lda + 8 * ((lane & 1) ^ ((r >> 3) & 1))) * 2;
  }
  // B copies: wave w = KiB (w & 3) of column block (w >> 2) of the half's group image (region 1: group gB)
  const char* bsrc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int gq = p.w_gstride ? (q ? gB : gA) : 0;
    bsrc[q] = reinterpret_cast<const char*>(p.bimg) +
              ((int64_t)gq * p.bimg_ntn + p.bimg_tn0 + 2 * tw + (wave >> 2)) * nk * PG_B_BYTES + (wave & 3) * 1024 +
              16 * lane;
  }
  auto issue = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ks = 2 * s + j;
      char* sb = lds + buf * STG + j * SUB;
      if (ABF) {
        __builtin_amdgcn_global_load_lds((const void*)(asrcb + 32 * ks), (lds_void_t*)(sb + wave * 1024), 16, 0, 0);
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + 16 * ks), (lds_void_t*)(sb + (2 * wave + i) * 1024),
                                           16, 0, 0);
      }
      __builtin_amdgcn_global_load_lds((const void*)(bsrc[0] + (int64_t)ks * PG_B_BYTES),
                                       (lds_void_t*)(sb + ABYTES + wave * 1024), 16, 0, 0);
      if (!uni)
        __builtin_amdgcn_global_load_lds((const void*)(bsrc[1] + (int64_t)ks * PG_B_BYTES),
                                         (lds_void_t*)(sb + ABYTES + 8192 + wave * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  int aoff0[4], aoff1[4], aoffb[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int ra = 128 * rh + 32 * m + li;
    aoff0[m] = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
    aoff1[m] = ra * 64 + 16 * ((2 * h + 1) ^ ((li >> 2) & 3));
    aoffb[m] = ra * 32 + 16 * (h ^ ((li >> 3) & 1));
  }
  const int boff = ABYTES + (uni ? 0 : rh * 8192) + (cq >> 1) * 4096 + 2048 * (cq & 1) + li * 32 + 16 * (h ^ ((li >> 3) & 1));

  bool xnw[4] = {};
  float xrs[4] = {};
  uint16_t* xnp[4] = {};
  float* gsm = reinterpret_cast<float*>(lds + NSTG * STG);
  if (RSC && p.xn_out && tw == 0) {
    for (int k = 4 * t; k < p.K; k += 4 * 512)
      *reinterpret_cast<f32x4*>(gsm + k) = *reinterpret_cast<const f32x4*>(p.a_gamma + k);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t xgr = (int64_t)tp * 2 * GT + 128 * rh + 32 * m + li;
      const int xir = p.in_rows ? p.in_rows[xgr] : (int)xgr;
      xnw[m] = xir >= 0 && cq == 0;
      if (xnw[m]) {
        xrs[m] = p.a_rstd[xir];
        xnp[m] = p.xn_out + (int64_t)xir * p.ldxn + 8 * h;
      }
    }
  }

  issue(0, 0);
  if (NSTG >= 3 && ns > 1) issue(1, 1);
  for (int s = 0; s < ns; ++s) {
    if (NSTG >= 3 && s + 1 < ns) {
      if (uni) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (AOPS + 1)) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (AOPS + 2)) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s + NSTG - 1 < ns) issue(s + NSTG - 1, (s + NSTG - 1) % NSTG);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ks = 2 * s + j;
      const char* sb = lds + (s % NSTG) * STG + j * SUB;
      u32x4 fb[2], fa[4];
#pragma unroll
      for (int n = 0; n < 2; ++n) fb[n] = *reinterpret_cast<const u32x4*>(sb + boff + n * 1024);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if constexpr (ABF) {
          fa[m] = *reinterpret_cast<const u32x4*>(sb + aoffb[m]);
          if (RSC && xnw[m]) {
            const float* gp = gsm + 16 * ks + 8 * h;
            const u32x4 w = fa[m];
            const f32x4 a0 = {__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                              __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
            const f32x4 a1 = {__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u),
                              __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
            const u32x2 b0 = bf16_rne4(a0 * *reinterpret_cast<const f32x4*>(gp) * xrs[m]);
            const u32x2 b1 = bf16_rne4(a1 * *reinterpret_cast<const f32x4*>(gp + 4) * xrs[m]);
            *reinterpret_cast<u32x4*>(xnp[m] + 16 * ks) = u32x4{b0.x, b0.y, b1.x, b1.y};
          }
        } else {
          const f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0[m]);
          const f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + aoff1[m]);
          const u32x2 b0 = bf16_rne4(a0), b1 = bf16_rne4(a1);
          fa[m] = u32x4{b0.x, b0.y, b1.x, b1.y};
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[2 * m + n] = mfma_bf16(fa[m], fb[n], acc[2 * m + n]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                    // the epilogue reuses the stage buffers
  // each row half's four waves finish its two quarters in its own LDS (both halves in step: same barriers)
  float* esm = smem + rh * (64 * (GT + 4) + 8 * GT);
  const int tm = 2 * tp + rh;
  const int g = rh ? gB : gA;
  gemm_vec_epilogue<EPIT, 4, RSC, OT_PLANE_EPI_RBN, true>(p, acc, esm, tm, n0, g, 0, t & 255);
  __syncthreads();
  gemm_vec_epilogue<EPIT, 4, RSC, OT_PLANE_EPI_RBN, true>(p, acc, esm, tm, n0 + GT, g, 1, t & 255);
}
#define OT_WIDE_LIST(X)                                                                        \
  X(OT_AX_NONE, 0)                                                                             \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)                           \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                                            \
  X(OT_AX_BF16_RMSNORM, 0)                                                                     \
  X(OT_AX_BF16_RMSNORM, OT_EPI_BIAS)                                                           \
  X(OT_AX_BF16_RMSNORM, OT_EPI_BIAS | OT_EPI_C_BF16)                                           \
  X(OT_AX_BF16, 0)                                                                             \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL)                                                 \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT)                                \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)              \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                               \
  X(OT_AX_BF16, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16 | OT_EPI_AUX_BF16)             \
  X(OT_AX_BF16, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16)                               \
  X(OT_AX_BF16, OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT)                                           \
  X(OT_AX_BF16, OT_EPI_RMSNORM_BWD)

// the tile for a bf16-mode plane GEMM of N % 256 == 0 columns (K % 32 == 0): measured at C5's shapes
// (tools/c5_gemm_bench.py, profiles/r06/c5_gemm_tiles.txt)
// (K >= N: 128 x 256 ~20% faster than 128 x 128 — C5's FFN2 / Wo forwards and input-gradient GEMMs; output-heavy
// shapes (N > K: FFN1 / QKV forwards, FFN2 dgrad) stay on 128 x 128, the 256-column tiles' epilogues serialise there;
// 256 x 256 and 128 x 512 measured slower at every C5 shape)
int plane_tile_auto(int K, int N, int ntiles) {
  (void)ntiles;
  return N <= K ? 1 : 0;
}

// process-wide switch of the wide tile (ot_plane_wide: A/B timing and the bit-identity tests)
static std::atomic<int> g_plane_wide{OT_PLANE_WIDE};
extern "C" int ot_plane_wide(int on) {
  const int prev = g_plane_wide.load();
  if (on >= 0) g_plane_wide.store(on > 4 ? 4 : on);
  return prev;
}

// the wide kernel for (a_xform, epi), or null; its stage LDS bytes in *stage_lds (opted in above 64 KiB once)
// kind 1: 128 x 256 (plane_wide_kernel), 2: 128 x 512 (plane_big_kernel), 3: 256 x 256 (plane_sq_kernel)
void (*plane_wide_for(int x, int e, int kind, int* stage_lds))(GemmArgs) {
  void (*k)(GemmArgs) = nullptr;
#define OT_WIDE_PICK(AX_, EP_)                                                                        \
  if (x == (AX_) && e == (EP_)) {                                                                     \
    k = kind == 3 ? plane_sq_kernel<AX_, EP_> : kind == 2 ? plane_big_kernel<AX_, EP_> : plane_wide_kernel<AX_, EP_>; \
    *stage_lds = kind == 3 ? ps_stage_lds<AX_>() : kind == 2 ? pb_stage_lds<AX_>() : pw_stage_lds<AX_>();  \
  }
  OT_WIDE_LIST(OT_WIDE_PICK)
#undef OT_WIDE_PICK
  static std::once_flag once;
  std::call_once(once, [] {
#define OT_WIDE_ATTR(AX_, EP_)                                                                               \
  (void)hipFuncSetAttribute((const void*)plane_wide_kernel<AX_, EP_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                            pw_stage_lds<AX_>() + 4096);                                                         \
  (void)hipFuncSetAttribute((const void*)plane_big_kernel<AX_, EP_>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                            pb_stage_lds<AX_>() + 4096);                                                        \
  (void)hipFuncSetAttribute((const void*)plane_sq_kernel<AX_, EP_>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                            ps_stage_lds<AX_>() + 4096);
    OT_WIDE_LIST(OT_WIDE_ATTR)
#undef OT_WIDE_ATTR
    (void)hipGetLastError();
  });
  return k;
}

}  // namespace ot
