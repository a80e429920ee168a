// Weight gradients of the grouped GEMM (ot_mixed_gemm_wgrad*): dW[g] (+)= sum_rows pro(A[a_row])^T D[d_row],
// db[g] (+)= sum_rows D[d_row], as per-chunk partial slabs and a deterministic reduce; and the transposed weight
// shadow the input-gradient GEMMs read (ot_transpose_banks).
#include <atomic>
#include <mutex>

#include "gemm.h"

namespace ot {

#ifndef OT_WGRAD_BF16_RS          // 32-row groups per stage of the bf16-mode weight-gradient kernel
#define OT_WGRAD_BF16_RS 2
#endif
constexpr int WGRAD_BF16_RS = OT_WGRAD_BF16_RS;
#ifndef OT_WGRAD_DBUF
#define OT_WGRAD_DBUF 0
#endif

// Weight-gradient tiles: whole row chunks per XCD.  Block b runs on XCD b % 8 (round-robin dispatch), so XCD x
// takes chunks x, x + 8, x + 16, ... and each chunk's (k, n) tiles occupy consecutive dispatch slots of that XCD:
// every tile of a chunk streams the same rows, and they are then read through one L2.  (The contiguous-range
// remap split chunks across two XCDs whenever a range was not a whole number of chunks: C5's W1 weight gradient
// fetched 2.3x its algorithmic bytes.)  The grid is padded to whole rounds of 8 chunks; padding blocks return.
// Fewer than 8 chunks (small batches): whole chunks per XCD would leave XCDs idle, so the tiles are dealt in
// order (block b = chunk b / per_chunk), spread over every XCD; the grid is then nchunks x per_chunk.
__host__ __device__ inline unsigned wgrad_grid(int nchunks, int per_chunk) {
  return (unsigned)(nchunks < 8 ? nchunks : (nchunks + 7) / 8 * 8) * per_chunk;
}
__device__ __forceinline__ bool wgrad_tile(int b, int per_chunk, int nchunks, int& c, int& rem) {
  if (nchunks < 8) {
    c = b / per_chunk;
    rem = b % per_chunk;
    return true;
  }
  const int x = b & 7, j = b >> 3;
  c = x + 8 * (j / per_chunk);
  rem = j % per_chunk;
  return c < nchunks;
}

// ------------------------------------------------------------------------------------------
// wgrad: partial slab per (chunk, k-tile, n-tile):  slab[c][k][n] = sum_{rows of chunk} A^T D
// LDS images are row-major, as loaded: As[r][k], Ds[r][n] (BR = 32 rows per stage, row stride 128,
// no padding): the staging stores are whole 16-B pieces of 512-B rows (conflict-free), and the
// MFMA operands need no transpose — the reduction row is the MFMA k index, so lane (li, h) of step
// s reads As[2s + h][k0 + li] (32 consecutive floats per half-wave: conflict-free ds_read_b32, two
// steps per ds_read2st64_b32).
constexpr int WBR = 32;
constexpr int WLD = GT;

struct WgradArgs {
  const float* A; int64_t lda; const int32_t* a_rows; int a_xform; const float* a_rstd; const float* a_gamma;
  const float* D; int64_t ldd; const int32_t* d_rows;
  int K, N;
  const int32_t* chunks;     // [nchunks*3] {group, row_begin, row_count} (rows index the row maps)
  int nchunks;
  float* slab;               // [nchunks][K][N]
  float* bslab;              // [nchunks][N] or null
  int ntk, ntn;
  // TERMS 2 (the scaled fp16 pair): bounds of |A| (null with the RMSNorm prologue: sqrt(K) |gamma_k| per column)
  // and |D|, one float each (ot_mixed_gemm_wgrad_ex)
  const float* a_bound; const float* d_bound;
  // OT_WG_D_KEEPBITS (the pair form with the GELU prologue): D is read unmasked and a row's dropout keep bits
  // [d_row][ldkeep] (bit n % 32 of word n / 32) select D' = keep ? D * d_scale : 0; d_bound then bounds |D| and the
  // kernel multiplies it by d_scale
  const uint32_t* keep; int64_t ldkeep; float d_scale;
};

template <int AXT>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // [NBUF][WBR][WLD] for A (r, k) then [NBUF][WBR][WLD] for D (r, n)
  const int ax = AXT >= 0 ? AXT : p.a_xform;
  const int per_chunk = p.ntk * p.ntn;
  // XCD-aware: the output tiles of one chunk (which share its A or D rows) get consecutive logical
  // ids, and xcd_remap places consecutive ids on one XCD, so the shared rows come from that L2
  int c, rem;
  if (!wgrad_tile(blockIdx.x, per_chunk, p.nchunks, c, rem)) return;
  const int tk = rem / p.ntn, tn = rem % p.ntn;
  const int k0 = tk * GT, n0 = tn * GT;
  const int row_begin = p.chunks[3 * c + 1], row_count = p.chunks[3 * c + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int sr = t >> 3, sc = t & 7;       // staging: row sr of the stage, float4 columns sc + 8i
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  float bsum = 0.f;
  const bool do_bias = p.bslab && tk == 0 && t < GT;

  // row indices of a stage, raw (the in-range test is applied in load_stage, one stage later, so
  // nothing waits on these loads before the MFMA block)
  auto rows_of = [&](int rs, int& ar, int& dr) {
    const int lr = rs + sr;
    const int64_t mi = (int64_t)row_begin + (lr < row_count ? lr : 0);
    ar = p.a_rows ? p.a_rows[mi] : (int)mi;
    dr = p.d_rows ? p.d_rows[mi] : (int)mi;
  };
  // raw branch-free loads (clamped addresses, masked at store time); the prologue transform runs in
  // store_stage so stage st+1's loads stay in flight across stage st's MFMAs
  f32x4 va[4], vd[4], gv[4];
  float rsd = 1.f;
  bool aok = false, dok = false;
  auto load_stage = [&](int st, int ar, int dr) {
    const bool in = st * WBR + sr < row_count && ar >= 0 && dr >= 0;
    aok = in; dok = in;
    const float* pa = p.A + (int64_t)(aok ? ar : 0) * p.lda;
    const float* pd = p.D + (int64_t)(dok ? dr : 0) * p.ldd;
    if (ax == OT_AX_RMSNORM) rsd = p.a_rstd[aok ? ar : 0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 4 * (sc + 8 * i), n = n0 + 4 * (sc + 8 * i);
      const int kc = k < p.K ? k : 0, nc = n < p.N ? n : 0;
      va[i] = *reinterpret_cast<const f32x4*>(pa + kc);
      vd[i] = *reinterpret_cast<const f32x4*>(pd + nc);
      if (ax == OT_AX_RMSNORM) gv[i] = *reinterpret_cast<const f32x4*>(p.a_gamma + kc);
    }
  };
  constexpr int NBUF = OT_WGRAD_DBUF ? 2 : 1;
  auto store_stage = [&](int buf) {
    float* As = smem + buf * WBR * WLD;
    float* Ds = smem + (NBUF + buf) * WBR * WLD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = 4 * (sc + 8 * i);
      f32x4 a = va[i], dv = vd[i];
      if (ax == OT_AX_RMSNORM) {
        a = a * gv[i] * rsd;
      } else if (ax == OT_AX_GELU) {
        a = gelu_erf4(a);
      }
      if (!(aok && k0 + kk < p.K)) a = zero4;
      if (!(dok && n0 + kk < p.N)) dv = zero4;
      *reinterpret_cast<f32x4*>(As + sr * WLD + kk) = a;
      *reinterpret_cast<f32x4*>(Ds + sr * WLD + kk) = dv;
    }
  };

  const int nst = (row_count + WBR - 1) / WBR;
  int ar, dr, ar2 = -1, dr2 = -1;
  rows_of(0, ar, dr);
  if (nst > 1) rows_of(WBR, ar2, dr2);
  load_stage(0, ar, dr);
  store_stage(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int cur = NBUF == 2 ? (st & 1) : 0;
    const bool more = st + 1 < nst;
    int ar3 = -1, dr3 = -1;
    if (more) {
      load_stage(st + 1, ar2, dr2);                       // stage st+1 data
      if (st + 2 < nst) rows_of((st + 2) * WBR, ar3, dr3);   // stage st+2 row indices
    }
    const float* As = smem + cur * WBR * WLD;
    const float* Ds = smem + (NBUF + cur) * WBR * WLD;
    if (do_bias) {
#pragma unroll
      for (int r = 0; r < WBR; r += 4)
        bsum += (Ds[r * WLD + t] + Ds[(r + 1) * WLD + t]) + (Ds[(r + 2) * WLD + t] + Ds[(r + 3) * WLD + t]);
    }
    // 16 MFMA k-steps over the 32 rows: step s takes rows 2s (lane half 0) and 2s + 1 (half 1)
    float fa[16][2], fb[16][2];
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2)
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        fa[s2][m] = As[(2 * s2 + h) * WLD + wm + 32 * m + li];
        fb[s2][m] = Ds[(2 * s2 + h) * WLD + wn + 32 * m + li];
      }
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s2][m], fb[s2][n], acc[m][n], 0, 0, 0);
    if (NBUF == 2) {
      if (more) store_stage(cur ^ 1);
      __syncthreads();
    } else {
      __syncthreads();
      if (more) store_stage(0);
      __syncthreads();
    }
    ar2 = ar3; dr2 = dr3;
  }
  float* slab = p.slab + (int64_t)c * p.K * p.N;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (k >= p.K) continue;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = n0 + wn + 32 * n + li;
        if (col < p.N) slab[(int64_t)k * p.N + col] = acc[m][n][r];
      }
    }
  if (do_bias && n0 + t < p.N) p.bslab[(int64_t)c * p.N + n0 + t] = bsum;
}

// ------------------------------------------------------------------------------------------
// Split-bf16 wgrad (OT_MATMUL_SPLIT_BF16): same chunk/slab contract as wgrad_kernel.  The 32-row
// stage of A and D is split into three bf16 planes stored ROW-major in LDS (the staging writes stay
// 8-B pieces of the loaded rows), and the MFMA operands, which need 8 consecutive data rows of one
// column per lane, come out of ds_read_b64_tr_b16 transposed reads (4 rows x 16 columns per 16-lane
// group).  Row images are 256 B with the 16-B chunk XOR swizzle ch ^ ((r&3)<<2 | (r>>2)&3), which
// makes both the staging writes and the transposed reads conflict-free (cdna_hip_programming T10).
typedef short v4i16 __attribute__((ext_vector_type(4)));
constexpr int WSPLANE = WBR * 256;          // bytes of one plane image (32 rows x 128 bf16)
constexpr int WSOP = 3 * WSPLANE;           // bytes of one operand (3 planes)

__device__ __forceinline__ int wsw_off(int r, int ch) { return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

__device__ __forceinline__ v4i16 ds_tr16(const char* base, int off) {
  typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(base + off));
}

// RS: 32-row groups per stage.  The bf16 mode (TERMS = 1: one plane, 8 MFMAs per 32 rows per wave) takes
// 64-row stages (RS = 2): twice the MFMAs between the stage's two barriers, the two row groups' planes in
// the space the split mode's three planes use (the swizzle depends on r & 15, so row r + 32 keeps it).
template <int TERMS>
constexpr int wgrad_rs() { return WGRAD_BF16_RS > 0 && TERMS == 1 ? WGRAD_BF16_RS : 1; }

// DBF: D holds bf16 values (OT_WG_D_BF16: the FFN2 dgrad's bf16 dU)
// TERMS 2: the scaled fp16 pair (two planes, three f16 products instead of six bf16): A column k scaled by s_k and D
// by t, powers of two from per-tensor bounds (p.a_bound / p.d_bound, written by the operands' producers; the
// RMSNorm prologue's A needs none: |x_k rstd gamma_k| <= sqrt(K) |gamma_k|), the accumulator unscaled by
// 1 / (s_k t) at the store.  Every element keeps 22 significant bits of itself down to 2^-16 of its bound (below,
// an absolute error under 2^-38 of the bound).
// KEEP: D masked at staging time from stored keep bits (OT_WG_D_KEEPBITS) — one 16-byte word per row and stage; no
// hashing here: every D element is read again by each of the K / 128 column-tile workgroups
template <int AXT, int TERMS, bool DBF = false, bool KEEP = false>
__global__ __launch_bounds__(256, 2) void wgrad_split_kernel(WgradArgs p) {
  constexpr int RS = wgrad_rs<TERMS>();
  static_assert(!KEEP || (TERMS == 2 && AXT == OT_AX_GELU && !DBF), "keep-bits D: the pair form of the W2 gradient");
  static_assert(RS * WSPLANE <= WSOP && (TERMS == 1 || RS == 1), "wgrad stage LDS");
  static_assert(TERMS != 2 || (!DBF && (AXT == OT_AX_NONE || AXT == OT_AX_RMSNORM || AXT == OT_AX_GELU)),
                "pair wgrad forms");
  constexpr bool PAIR = TERMS == 2;
  constexpr int BR = WBR * RS;                   // rows per stage
  constexpr int NPL = TERMS == 1 ? 1 : PAIR ? 2 : 3;
  extern __shared__ __attribute__((aligned(16))) char smem_c[];
  const int ax = AXT >= 0 ? AXT : p.a_xform;
  const int per_chunk = p.ntk * p.ntn;
  int c, rem;
  if (!wgrad_tile(blockIdx.x, per_chunk, p.nchunks, c, rem)) return;
  const int tk = rem / p.ntn, tn = rem % p.ntn;
  const int k0 = tk * GT, n0 = tn * GT;
  const int row_begin = p.chunks[3 * c + 1], row_count = p.chunks[3 * c + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int sr = t >> 3, sc = t & 7;       // staging: rows sr + 32 j of the stage, float4 columns sc + 8i
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  char* As = smem_c;
  char* Ds = smem_c + WSOP;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  const bool do_bias = p.bslab && tk == 0;
  f32x4 bsum[4] = {zero4, zero4, zero4, zero4};
  f32x4 gv[4];                                   // RMSNorm gamma of this thread's k columns (stage-invariant)
  if (ax == OT_AX_RMSNORM) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 4 * (sc + 8 * i);
      gv[i] = *reinterpret_cast<const f32x4*>(p.a_gamma + (k < p.K ? k : 0));
    }
  }
  // TERMS 2: this thread's column scales of A (k columns 4 (sc + 8 i) ..) and D's scale
  f32x4 sa[4];
  float sdv = 1.f;
  if constexpr (PAIR) {
    sdv = pow2_scale14(KEEP ? p.d_bound[0] * p.d_scale : p.d_bound[0]);
    const float sqk = sqrtf((float)p.K);
    const float s1 = AXT == OT_AX_RMSNORM ? 1.f : pow2_scale14(p.a_bound[0]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sa[i] = AXT == OT_AX_RMSNORM
                  ? f32x4{pow2_scale14(sqk * fabsf(gv[i].x)), pow2_scale14(sqk * fabsf(gv[i].y)),
                          pow2_scale14(sqk * fabsf(gv[i].z)), pow2_scale14(sqk * fabsf(gv[i].w))}
                  : f32x4{s1, s1, s1, s1};
  }

  auto rows_of = [&](int rs, int (&ar)[RS], int (&dr)[RS]) {
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      const int lr = rs + sr + WBR * j;
      const int64_t mi = (int64_t)row_begin + (lr < row_count ? lr : 0);
      ar[j] = p.a_rows ? p.a_rows[mi] : (int)mi;
      dr[j] = p.d_rows ? p.d_rows[mi] : (int)mi;
    }
  };
  f32x4 va[RS][4], vd[RS][4];
  float rsd[RS];
  bool inr[RS];
  u32x4 kw[RS];                                  // KEEP: the 128 keep bits of this thread's D row (columns n0 ..)
  auto load_stage = [&](int st, const int (&ar)[RS], const int (&dr)[RS]) {
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      inr[j] = st * BR + sr + WBR * j < row_count && ar[j] >= 0 && dr[j] >= 0;
      const float* pa = p.A + (int64_t)(inr[j] ? ar[j] : 0) * p.lda;
      const uint16_t* pa16 = reinterpret_cast<const uint16_t*>(p.A) + (int64_t)(inr[j] ? ar[j] : 0) * p.lda;
      const float* pd = p.D + (int64_t)(inr[j] ? dr[j] : 0) * p.ldd;
      rsd[j] = ax == OT_AX_RMSNORM ? p.a_rstd[inr[j] ? ar[j] : 0] : 1.f;
      if constexpr (KEEP)
        kw[j] = *reinterpret_cast<const u32x4*>(p.keep + (int64_t)(inr[j] ? dr[j] : 0) * p.ldkeep + (n0 >> 5));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * (sc + 8 * i), n = n0 + 4 * (sc + 8 * i);
        const int kc = k < p.K ? k : 0, nc = n < p.N ? n : 0;
        if (AXT == OT_AX_BF16) {                       // bf16 values: exact in f32 (and in the planes)
          const u32x2 w = *reinterpret_cast<const u32x2*>(pa16 + kc);
          va[j][i] = f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                           __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
        } else {
          va[j][i] = *reinterpret_cast<const f32x4*>(pa + kc);
        }
        if (DBF) {
          const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.D) +
                                                          (int64_t)(inr[j] ? dr[j] : 0) * p.ldd + nc);
          vd[j][i] = f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                           __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
        } else {
          vd[j][i] = *reinterpret_cast<const f32x4*>(pd + nc);
        }
      }
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int j = 0; j < RS; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cc = sc + 8 * i;                      // float4 column index 0..31
        f32x4 a = va[j][i], dv = vd[j][i];
        if (ax == OT_AX_RMSNORM) {
          a = a * gv[i] * rsd[j];
        } else if (ax == OT_AX_GELU) {
          a = gelu_erf4(a);
        }
        // only D is zeroed, for rows past the chunk or with a negative id: their A (row 0 of the map, clamped
        // columns) is finite, so its products are 0; columns past K / N feed outputs that are never stored
        // (a 0 / 1 row factor: four multiplies, no compare-and-select chain).  Finiteness assumption: row 0 of A
        // and D must be finite — a non-finite value there (a diverged step) turns the padding rows' 0 * inf into
        // NaN in every dW tile and bias sum of a chunk with padding, where selects would have kept it to the rows
        // that hold it.  A diverged step's gradients are NaN anyway; bench.py refuses to time non-finite steps.
        if constexpr (KEEP) {                           // float4 i holds columns 32 i + 4 sc ..: word i, nibble sc
          // keep ? d * scale : 0 as (d & -bit) * scale
          const int nb = (int)(kw[j][i] >> (4 * sc));
          auto kept = [&](float v, int e) {
            return __uint_as_float(__float_as_uint(v) & (uint32_t)((nb << (31 - e)) >> 31));
          };
          dv = f32x4{kept(dv.x, 0), kept(dv.y, 1), kept(dv.z, 2), kept(dv.w, 3)} * p.d_scale;
        }
        dv = dv * (inr[j] ? 1.f : 0.f);
        bsum[i] += dv;                                  // (unconditional: cheaper than the if-converted select;
                                                        // stored only when do_bias)
        const int off = wsw_off(sr + WBR * j, cc >> 1) + 8 * (cc & 1);
        if constexpr (TERMS == 1) {
          *reinterpret_cast<u32x2*>(As + off) = bf16_rne4(a);
          *reinterpret_cast<u32x2*>(Ds + off) = bf16_rne4(dv);
          continue;
        }
        if constexpr (PAIR) {
          u32x2 h0, l0;
          pair4(a * sa[i], h0, l0);
          *reinterpret_cast<u32x2*>(As + off) = h0;
          *reinterpret_cast<u32x2*>(As + WSPLANE + off) = l0;
          pair4(dv * sdv, h0, l0);
          *reinterpret_cast<u32x2*>(Ds + off) = h0;
          *reinterpret_cast<u32x2*>(Ds + WSPLANE + off) = l0;
          continue;
        }
        u32x2 q0, q1, q2;
        split3(a, q0, q1, q2);
        *reinterpret_cast<u32x2*>(As + off) = q0;
        *reinterpret_cast<u32x2*>(As + WSPLANE + off) = q1;
        *reinterpret_cast<u32x2*>(As + 2 * WSPLANE + off) = q2;
        split3(dv, q0, q1, q2);
        *reinterpret_cast<u32x2*>(Ds + off) = q0;
        *reinterpret_cast<u32x2*>(Ds + WSPLANE + off) = q1;
        *reinterpret_cast<u32x2*>(Ds + 2 * WSPLANE + off) = q2;
      }
  };
  // transposed-read addresses (stage-invariant): lane 4q+pp of its 16-lane group reads row
  // r0 + q, chunk c0 + (pp >> 1), half pp & 1; r0 = 16 t2 + 8 h + 4 rd, c0 = (col0 + 16 (g & 1)) / 8
  const int gi = lane & 15, q = gi >> 2, pp = gi & 3, g1 = (lane >> 4) & 1;
  int aoff[2][2], doff[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int r = 8 * h + 4 * rd + q;
      aoff[m][rd] = wsw_off(r, (wm + 32 * m + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
      doff[m][rd] = wsw_off(r, (wn + 32 * m + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
    }

  const int nst = (row_count + BR - 1) / BR;
  int ar[RS], dr[RS], ar2[RS], dr2[RS];
  rows_of(0, ar, dr);
  if (nst > 1) rows_of(BR, ar2, dr2);
  load_stage(0, ar, dr);
  store_stage();
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const bool more = st + 1 < nst;
    int ar3[RS], dr3[RS];
    if (more) {
      load_stage(st + 1, ar2, dr2);
      if (st + 2 < nst) rows_of((st + 2) * BR, ar3, dr3);
    }
#pragma unroll
    for (int t2 = 0; t2 < 2 * RS; ++t2) {               // 16-row MFMA k-steps of the stage
      u32x4 fa[2][3], fb[2][3];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          const int po = pl * WSPLANE + t2 * 16 * 256;   // row r -> r + 16 keeps the swizzle (r & 15)
          const v4i16 a0 = ds_tr16(As + po, aoff[m][0]), a1 = ds_tr16(As + po, aoff[m][1]);
          const v4i16 d0 = ds_tr16(Ds + po, doff[m][0]), d1 = ds_tr16(Ds + po, doff[m][1]);
          const u32x2 a0u = __builtin_bit_cast(u32x2, a0), a1u = __builtin_bit_cast(u32x2, a1);
          const u32x2 d0u = __builtin_bit_cast(u32x2, d0), d1u = __builtin_bit_cast(u32x2, d1);
          fa[m][pl] = u32x4{a0u.x, a0u.y, a1u.x, a1u.y};
          fb[m][pl] = u32x4{d0u.x, d0u.y, d1u.x, d1u.y};
        }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if constexpr (TERMS == 1) {
            acc[m][n] = mfma_bf16(fa[m][0], fb[n][0], acc[m][n]);
            continue;
          }
          if constexpr (PAIR) {
            acc[m][n] = mfma_f16(fa[m][0], fb[n][1], acc[m][n]);
            acc[m][n] = mfma_f16(fa[m][1], fb[n][0], acc[m][n]);
            acc[m][n] = mfma_f16(fa[m][0], fb[n][0], acc[m][n]);
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
    }
    __syncthreads();
    if (more) store_stage();
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RS; ++j) { ar2[j] = ar3[j]; dr2[j] = dr3[j]; }
  }
  float* slab = p.slab + (int64_t)c * p.K * p.N;
  float ainv1 = 1.f;                                  // TERMS 2: 1 / (s_k t), exact powers of two
  if constexpr (PAIR) ainv1 = 1.f / ((AXT == OT_AX_RMSNORM ? 1.f : pow2_scale14(p.a_bound[0])) * sdv);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (k >= p.K) continue;
      float un = ainv1;
      if (PAIR && AXT == OT_AX_RMSNORM) un = 1.f / (pow2_scale14(sqrtf((float)p.K) * fabsf(p.a_gamma[k])) * sdv);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = n0 + wn + 32 * n + li;
        if (col < p.N) slab[(int64_t)k * p.N + col] = PAIR ? acc[m][n][r] * un : acc[m][n][r];
      }
    }
  if (do_bias) {
    // per-thread column partials (columns 4(sc + 8i)) -> LDS [sr][32 float4] -> fixed-order sum over
    // the 32 staging rows per column
    f32x4* bl = reinterpret_cast<f32x4*>(smem_c);
#pragma unroll
    for (int i = 0; i < 4; ++i) bl[sr * 32 + sc + 8 * i] = bsum[i];
    __syncthreads();
    if (t < GT && n0 + t < p.N) {
      const float* bf = reinterpret_cast<const float*>(smem_c);
      float a = 0.f;
      for (int r = 0; r < WBR; ++r) a += bf[r * GT + t];
      p.bslab[(int64_t)c * p.N + n0 + t] = a;
    }
  }
}


// Weight gradient with both operands in bf16 (a_xform OT_AX_BF16 | OT_WG_D_BF16, OT_MATMUL_BF16: the stored
// normalised inputs / GELU and the bf16 dU / dQKV).  The stage images are plain copies of the rows, so they
// go global -> LDS by global_load_lds straight into the swizzled layout the transposed fragment reads use
// (no VGPR staging, no conversion) through a ring of WG_NST 32-row stages, WG_NST - 1 of them in flight
// (the register-staged kernel keeps one; it waits on load latency, not MFMA: 10% MFMA busy at C5).  The
// row indices of a stage are loaded one iteration before its copies are issued.  Rows past the chunk or
// with a negative row index read a zero D row (A x 0 = 0; their A source is row 0, finite).  Columns past
// K / N read column 0 (their outputs are not stored).  IDL: row maps given (a_rows == d_rows).
#ifndef OT_WGRAD_NST
#define OT_WGRAD_NST 4
#endif
#ifndef OT_WGRAD_SR
#define OT_WGRAD_SR 32                            // rows per stage (16 or 32)
#endif
#ifndef OT_WGRAD_COPY_MINW
#define OT_WGRAD_COPY_MINW 2
#endif
constexpr int WG_NST = OT_WGRAD_NST;
constexpr int WG_SR = OT_WGRAD_SR;
constexpr int WG_NI = WG_SR / 16;                 // copies per wave per operand and stage (4 rows each)
constexpr int WG_IMG = WG_SR * 256;               // one stage's rows x 128-column bf16 image
constexpr int WG_STB = 2 * WG_IMG;                // A + D per stage
static_assert(WG_SR == 16 || WG_SR == 32, "copy-staged wgrad stage rows");
constexpr int WG_IDB = 16;                        // loop iterations per row-id block
constexpr int WG_IDR = WG_IDB * WG_SR;            // ids per block (a multiple of 256: two / thread at SR 32)
constexpr int WG_LDS = WG_NST * WG_STB + 2 * WG_IDR * 4;
__device__ __attribute__((aligned(16))) uint16_t g_zero_row[GT];   // zero-initialised with the module

// ds_read_b64_tr_b16 as inline asm: the intrinsic makes the compiler wait for every outstanding
// global_load_lds (vmcnt(0)) before it, which would drain the copy ring each stage.  The caller waits for
// the results itself (tr16_wait) before using them.
__device__ __forceinline__ v4i16 ds_tr16_nowait(const char* base, int off) {
  typedef __attribute__((address_space(3))) const char lds_cchar;
  const uint32_t a = (uint32_t)(uintptr_t)(lds_cchar*)(base + off);
  v4i16 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(a) : "memory");
  return r;
}
__device__ __forceinline__ void tr16_wait(v4i16& a, v4i16& b, v4i16& c, v4i16& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) :: "memory");
}

template <bool IDL>
__global__ __launch_bounds__(256, OT_WGRAD_COPY_MINW) void wgrad_bf16_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_c[];
  const int per_chunk = p.ntk * p.ntn;
  int c, rem;
  if (!wgrad_tile(blockIdx.x, per_chunk, p.nchunks, c, rem)) return;
  const int tk = rem / p.ntn, tn = rem % p.ntn;
  const int k0 = tk * GT, n0 = tn * GT;
  const int row_begin = p.chunks[3 * c + 1], row_count = p.chunks[3 * c + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A);
  const uint16_t* D16 = reinterpret_cast<const uint16_t*>(p.D);
  // copy lanes: instruction i of wave w fills image bytes [(2w + i) KiB, +1 KiB) = row 4 (2w + i) + lane / 16,
  // physical 16-B chunk lane % 16 = logical chunk (lane % 16) ^ swizzle(row) (wsw_off)
  int lrow[WG_NI], acol[WG_NI], dcol[WG_NI];
#pragma unroll
  for (int i = 0; i < WG_NI; ++i) {
    const int r = 4 * (WG_NI * wave + i) + (lane >> 4);
    const int lc = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
    lrow[i] = r;
    acol[i] = k0 + 8 * lc < p.K ? k0 + 8 * lc : 0;
    dcol[i] = n0 + 8 * lc < p.N ? n0 + 8 * lc : 0;
  }
  const int nst = (row_count + WG_SR - 1) / WG_SR;
  auto row_id = [&](int st, int i) -> int {           // direct lookup (prologue; identity maps)
    const int r = st * WG_SR + lrow[i];
    const int64_t mi = (int64_t)row_begin + (r < row_count ? r : 0);
    return IDL ? p.a_rows[mi] : (int)mi;
  };
  // Row-id blocks (row maps): the ids of the copies issued in iterations [16 b, 16 b + 16) — stages
  // 16 b + NST - 1 .. + 15 — go through an LDS double buffer behind the ring, loaded into registers one block
  // ahead and written at the block's first iteration.  (An id load per stage in the loop made the compiler
  // wait for every outstanding copy before the copies that use it.)
  int* idbuf = reinterpret_cast<int*>(smem_c + WG_NST * WG_STB);   // [2][WG_IDR]
  int pre[WG_IDR / 256];
  auto prefetch_block = [&](int b) {
#pragma unroll
    for (int j = 0; j < WG_IDR / 256; ++j) {
      const int r = (WG_IDB * b + WG_NST - 1) * WG_SR + t + 256 * j;
      const int64_t mi = (int64_t)row_begin + (r < row_count ? r : 0);
      pre[j] = p.a_rows[mi];
    }
  };
  auto issue = [&](int st, const int (&ids)[WG_NI]) {
    char* sb = smem_c + (st % WG_NST) * WG_STB;
#pragma unroll
    for (int i = 0; i < WG_NI; ++i) {
      const bool ok = st * WG_SR + lrow[i] < row_count && ids[i] >= 0;
      const uint16_t* sa = A16 + (int64_t)(ok ? ids[i] : 0) * p.lda + acol[i];
      const uint16_t* sd = ok ? D16 + (int64_t)ids[i] * p.ldd + dcol[i] : g_zero_row + 8 * (lane & 15);
      __builtin_amdgcn_global_load_lds((const void*)sa, (lds_void_t*)(sb + (WG_NI * wave + i) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)sd, (lds_void_t*)(sb + WG_IMG + (WG_NI * wave + i) * 1024), 16,
                                       0, 0);
    }
  };
  // transposed-read addresses, as in wgrad_split_kernel
  const int gi = lane & 15, q = gi >> 2, pp = gi & 3, g1 = (lane >> 4) & 1;
  int aoff[2][2], doff[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int r = 8 * h + 4 * rd + q;
      aoff[m][rd] = wsw_off(r, (wm + 32 * m + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
      doff[m][rd] = wsw_off(r, (wn + 32 * m + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
    }
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  // bias (tk == 0): thread t sums columns 2 (t & 63) + {0, 1} over rows (SR / 4) (t >> 6) .. of every stage
  const bool do_bias = p.bslab && tk == 0;
  const int bcp = t & 63, brs = t >> 6;
  float bs0 = 0.f, bs1 = 0.f;

  for (int s0 = 0; s0 < WG_NST - 1; ++s0)
    if (s0 < nst) {
      int ids[WG_NI];
#pragma unroll
      for (int i = 0; i < WG_NI; ++i) ids[i] = row_id(s0, i);
      issue(s0, ids);
    }
  if (IDL) prefetch_block(0);
  // in flight after stage st's copies when its wait comes: the copies of the NST - 2 stages issued after it
  // (vector memory loads retire in issue order; the id-block loads only add to the count, so the wait
  // is conservative around them)
  for (int st = 0; st < nst; ++st) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (st + WG_NST - 1 <= nst) {
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"((WG_NST - 2) * 2 * WG_NI) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const bool blk = IDL && (st % WG_IDB) == 0;
    if (blk) {                                        // this block's ids into LDS
      int* ib = idbuf + ((st / WG_IDB) & 1) * WG_IDR;
#pragma unroll
      for (int j = 0; j < WG_IDR / 256; ++j) ib[t + 256 * j] = pre[j];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();                     // every wave's copies of stage st are in; slot
    asm volatile("" ::: "memory");                    // (st - 1) % NST is no longer read
    if (blk) prefetch_block(st / WG_IDB + 1);
    if (st + WG_NST - 1 < nst) {
      int ids[WG_NI];
      const int* ib = idbuf + ((st / WG_IDB) & 1) * WG_IDR + (st % WG_IDB) * WG_SR;
#pragma unroll
      for (int i = 0; i < WG_NI; ++i) ids[i] = IDL ? ib[lrow[i]] : row_id(st + WG_NST - 1, i);
      issue(st + WG_NST - 1, ids);
    }
    const char* As = smem_c + (st % WG_NST) * WG_STB;
    const char* Ds = As + WG_IMG;
    if (do_bias) {
#pragma unroll
      for (int r8 = 0; r8 < WG_SR / 4; ++r8) {
        const int r = (WG_SR / 4) * brs + r8;
        const uint32_t w = *reinterpret_cast<const uint32_t*>(Ds + wsw_off(r, bcp >> 2) + 4 * (bcp & 3));
        bs0 += __uint_as_float(w << 16);
        bs1 += __uint_as_float(w & 0xffff0000u);
      }
    }
#pragma unroll
    for (int t2 = 0; t2 < WG_SR / 16; ++t2) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int po = t2 * 16 * 256;
        v4i16 a0 = ds_tr16_nowait(As + po, aoff[m][0]), a1 = ds_tr16_nowait(As + po, aoff[m][1]);
        v4i16 d0 = ds_tr16_nowait(Ds + po, doff[m][0]), d1 = ds_tr16_nowait(Ds + po, doff[m][1]);
        tr16_wait(a0, a1, d0, d1);
        const u32x2 a0u = __builtin_bit_cast(u32x2, a0), a1u = __builtin_bit_cast(u32x2, a1);
        const u32x2 d0u = __builtin_bit_cast(u32x2, d0), d1u = __builtin_bit_cast(u32x2, d1);
        fa[m] = u32x4{a0u.x, a0u.y, a1u.x, a1u.y};
        fb[m] = u32x4{d0u.x, d0u.y, d1u.x, d1u.y};
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = mfma_bf16(fa[m], fb[n], acc[m][n]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float* slab = p.slab + (int64_t)c * p.K * p.N;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (k >= p.K) continue;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = n0 + wn + 32 * n + li;
        if (col < p.N) slab[(int64_t)k * p.N + col] = acc[m][n][r];
      }
    }
  if (do_bias) {                                      // fixed-order sum of the 4 row sets per column
    __syncthreads();                                  // every wave is done with the ring
    float* bl = reinterpret_cast<float*>(smem_c);     // [4][128]
    bl[brs * GT + 2 * bcp] = bs0;
    bl[brs * GT + 2 * bcp + 1] = bs1;
    __syncthreads();
    if (t < GT && n0 + t < p.N)
      p.bslab[(int64_t)c * p.N + n0 + t] = ((bl[t] + bl[GT + t]) + bl[2 * GT + t]) + bl[3 * GT + t];
  }
}

// The copy-staged bf16 weight gradient on 128 (k) x 256 (n) output tiles (N % 256 == 0): a stage is the A image
// and two 128-column D images (24 KiB at 32 rows, three stages: two workgroups per CU), each wave 64 k x 128 n
// (one D image, 8 MFMAs per 16 rows against 4), 384 B of L2 -> LDS traffic per MFMA against 512.  Same
// products in the same row order as wgrad_bf16_kernel: the slabs are bit-identical.
#ifndef OT_WGRAD_WIDE
#define OT_WGRAD_WIDE 1                                 // auto: 256 x 256 where K and N allow, else 128 x 256
#endif
constexpr int WW_NST = 3;
constexpr int WW_STB = 3 * WG_IMG;
constexpr int WW_LDS = WW_NST * WW_STB + 2 * WG_IDR * 4;
template <bool IDL>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_wide_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_c[];
  const int ntw = p.N / (2 * GT);
  const int per_chunk = p.ntk * ntw;
  int c, rem;
  if (!wgrad_tile(blockIdx.x, per_chunk, p.nchunks, c, rem)) return;
  const int tk = rem / ntw, tw = rem % ntw;
  const int k0 = tk * GT, n0 = tw * 2 * GT;
  const int row_begin = p.chunks[3 * c + 1], row_count = p.chunks[3 * c + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int wm = (wave >> 1) * 64, wh = wave & 1;
  const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A);
  const uint16_t* D16 = reinterpret_cast<const uint16_t*>(p.D);
  int lrow[WG_NI], acol[WG_NI], dcol[WG_NI];
#pragma unroll
  for (int i = 0; i < WG_NI; ++i) {
    const int r = 4 * (WG_NI * wave + i) + (lane >> 4);
    const int lc = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
    lrow[i] = r;
    acol[i] = k0 + 8 * lc < p.K ? k0 + 8 * lc : 0;
    dcol[i] = n0 + 8 * lc;                              // (+ 128 for the second image; N % 256 == 0)
  }
  const int nst = (row_count + WG_SR - 1) / WG_SR;
  auto row_id = [&](int st, int i) -> int {
    const int r = st * WG_SR + lrow[i];
    const int64_t mi = (int64_t)row_begin + (r < row_count ? r : 0);
    return IDL ? p.a_rows[mi] : (int)mi;
  };
  int* idbuf = reinterpret_cast<int*>(smem_c + WW_NST * WW_STB);   // [2][WG_IDR]
  int pre[WG_IDR / 256];
  auto prefetch_block = [&](int b) {
#pragma unroll
    for (int j = 0; j < WG_IDR / 256; ++j) {
      const int r = (WG_IDB * b + WW_NST - 1) * WG_SR + t + 256 * j;
      const int64_t mi = (int64_t)row_begin + (r < row_count ? r : 0);
      pre[j] = p.a_rows[mi];
    }
  };
  auto issue = [&](int st, const int (&ids)[WG_NI]) {
    char* sb = smem_c + (st % WW_NST) * WW_STB;
#pragma unroll
    for (int i = 0; i < WG_NI; ++i) {
      const bool ok = st * WG_SR + lrow[i] < row_count && ids[i] >= 0;
      const uint16_t* sa = A16 + (int64_t)(ok ? ids[i] : 0) * p.lda + acol[i];
      const uint16_t* sd = ok ? D16 + (int64_t)ids[i] * p.ldd + dcol[i] : g_zero_row + 8 * (lane & 15);
      const int o = (WG_NI * wave + i) * 1024;
      __builtin_amdgcn_global_load_lds((const void*)sa, (lds_void_t*)(sb + o), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)sd, (lds_void_t*)(sb + WG_IMG + o), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(ok ? sd + GT : sd), (lds_void_t*)(sb + 2 * WG_IMG + o), 16, 0, 0);
    }
  };
  const int gi = lane & 15, q = gi >> 2, pp = gi & 3, g1 = (lane >> 4) & 1;
  int aoff[2][2], doff[4][2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int r = 8 * h + 4 * rd + q;
#pragma unroll
    for (int m = 0; m < 2; ++m) aoff[m][rd] = wsw_off(r, (wm + 32 * m + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) doff[nb][rd] = wsw_off(r, (32 * nb + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
  }
  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  // bias (tk == 0): thread t sums columns 4 (t & 63) .. + 3 (image (t & 63) >> 5) over rows (SR / 4) (t >> 6) ..
  const bool do_bias = p.bslab && tk == 0;
  const int bcp = t & 63, brs = t >> 6;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};

  for (int s0 = 0; s0 < WW_NST - 1; ++s0)
    if (s0 < nst) {
      int ids[WG_NI];
#pragma unroll
      for (int i = 0; i < WG_NI; ++i) ids[i] = row_id(s0, i);
      issue(s0, ids);
    }
  if (IDL) prefetch_block(0);
  for (int st = 0; st < nst; ++st) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (st + WW_NST - 1 <= nst) {
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"((WW_NST - 2) * 3 * WG_NI) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const bool blk = IDL && (st % WG_IDB) == 0;
    if (blk) {
      int* ib = idbuf + ((st / WG_IDB) & 1) * WG_IDR;
#pragma unroll
      for (int j = 0; j < WG_IDR / 256; ++j) ib[t + 256 * j] = pre[j];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (blk) prefetch_block(st / WG_IDB + 1);
    if (st + WW_NST - 1 < nst) {
      int ids[WG_NI];
      const int* ib = idbuf + ((st / WG_IDB) & 1) * WG_IDR + (st % WG_IDB) * WG_SR;
#pragma unroll
      for (int i = 0; i < WG_NI; ++i) ids[i] = IDL ? ib[lrow[i]] : row_id(st + WW_NST - 1, i);
      issue(st + WW_NST - 1, ids);
    }
    const char* As = smem_c + (st % WW_NST) * WW_STB;
    const char* Ds = As + WG_IMG * (1 + wh);
    if (do_bias) {
      const char* Db = As + WG_IMG * (1 + (bcp >> 5));
      const int bc = 4 * (bcp & 31);
#pragma unroll
      for (int r8 = 0; r8 < WG_SR / 4; ++r8) {
        const int r = (WG_SR / 4) * brs + r8;
        const u32x2 w = *reinterpret_cast<const u32x2*>(Db + wsw_off(r, bc >> 3) + 2 * (bc & 7));
        bs[0] += __uint_as_float(w.x << 16);
        bs[1] += __uint_as_float(w.x & 0xffff0000u);
        bs[2] += __uint_as_float(w.y << 16);
        bs[3] += __uint_as_float(w.y & 0xffff0000u);
      }
    }
#pragma unroll
    for (int t2 = 0; t2 < WG_SR / 16; ++t2) {
      const int po = t2 * 16 * 256;
      u32x4 fa[2], fb[4];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        v4i16 a0 = ds_tr16_nowait(As + po, aoff[m][0]), a1 = ds_tr16_nowait(As + po, aoff[m][1]);
        v4i16 d0 = ds_tr16_nowait(Ds + po, doff[2 * m][0]), d1 = ds_tr16_nowait(Ds + po, doff[2 * m][1]);
        v4i16 e0 = ds_tr16_nowait(Ds + po, doff[2 * m + 1][0]), e1 = ds_tr16_nowait(Ds + po, doff[2 * m + 1][1]);
        tr16_wait(a0, a1, d0, d1);
        asm volatile("" : "+v"(e0), "+v"(e1) :: "memory");   // (complete: the wait above is lgkmcnt(0))
        const u32x2 a0u = __builtin_bit_cast(u32x2, a0), a1u = __builtin_bit_cast(u32x2, a1);
        const u32x2 d0u = __builtin_bit_cast(u32x2, d0), d1u = __builtin_bit_cast(u32x2, d1);
        const u32x2 e0u = __builtin_bit_cast(u32x2, e0), e1u = __builtin_bit_cast(u32x2, e1);
        fa[m] = u32x4{a0u.x, a0u.y, a1u.x, a1u.y};
        fb[2 * m] = u32x4{d0u.x, d0u.y, d1u.x, d1u.y};
        fb[2 * m + 1] = u32x4{e0u.x, e0u.y, e1u.x, e1u.y};
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = mfma_bf16(fa[m], fb[n], acc[m][n]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float* slab = p.slab + (int64_t)c * p.K * p.N;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (k >= p.K) continue;
#pragma unroll
      for (int n = 0; n < 4; ++n) slab[(int64_t)k * p.N + n0 + GT * wh + 32 * n + li] = acc[m][n][r];
    }
  if (do_bias) {                                      // fixed-order sum of the 4 row sets per column
    __syncthreads();
    float* bl = reinterpret_cast<float*>(smem_c);     // [4][256]
#pragma unroll
    for (int j = 0; j < 4; ++j) bl[brs * 2 * GT + 4 * bcp + j] = bs[j];
    __syncthreads();
    p.bslab[(int64_t)c * p.N + n0 + t] = ((bl[t] + bl[2 * GT + t]) + bl[4 * GT + t]) + bl[6 * GT + t];
  }
}

// The copy-staged bf16 weight gradient on 256 x 256 output tiles (K % 256 == 0, N % 256 == 0): 8 waves, wave
// (wk, wn) = k rows 64 wk .. + 63 x n columns 128 wn .. + 127; a 32-row stage is four 128-column images (A 0 / 1,
// D 0 / 1; 32 KiB), four stages (three in flight); 256 B of L2 -> LDS per MFMA.  Same products in the same row order
// as wgrad_bf16_kernel (bias: the first 256 threads, as wgrad_bf16_wide_kernel): the slabs are bit-identical.
constexpr int WS_NST = 4;
constexpr int WS_STB = 4 * WG_IMG;
constexpr int WS_IDR = WG_IDB * WG_SR;                 // ids per block: one per thread (512)
constexpr int WS_LDS = WS_NST * WS_STB + 2 * WS_IDR * 4;
static_assert(WG_SR == 32 && WS_IDR == 512, "square wgrad: 32-row stages");
template <bool IDL>
__global__ __launch_bounds__(512, 1) void wgrad_bf16_sq_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_c[];
  const int ntw = p.N / (2 * GT), ntk = p.K / (2 * GT);
  const int per_chunk = ntk * ntw;
  int c, rem;
  if (!wgrad_tile(blockIdx.x, per_chunk, p.nchunks, c, rem)) return;
  const int tk = rem / ntw, tw = rem % ntw;
  const int k0 = tk * 2 * GT, n0 = tw * 2 * GT;
  const int row_begin = p.chunks[3 * c + 1], row_count = p.chunks[3 * c + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int wk = wave >> 1, wn = wave & 1;
  const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A);
  const uint16_t* D16 = reinterpret_cast<const uint16_t*>(p.D);
  // copy lanes: wave w fills KiB w of each image = rows 4 w + lane / 16, physical chunk lane % 16
  const int lrow = 4 * wave + (lane >> 4);
  const int lc = (lane & 15) ^ (((lrow & 3) << 2) | ((lrow >> 2) & 3));
  const int acol = k0 + 8 * lc, dcol = n0 + 8 * lc;
  const int nst = (row_count + WG_SR - 1) / WG_SR;
  auto row_id = [&](int st) -> int {
    const int r = st * WG_SR + lrow;
    const int64_t mi = (int64_t)row_begin + (r < row_count ? r : 0);
    return IDL ? p.a_rows[mi] : (int)mi;
  };
  int* idbuf = reinterpret_cast<int*>(smem_c + WS_NST * WS_STB);   // [2][WS_IDR]
  int pre = 0;
  auto prefetch_block = [&](int b) {
    const int r = (WG_IDB * b + WS_NST - 1) * WG_SR + t;
    const int64_t mi = (int64_t)row_begin + (r < row_count ? r : 0);
    pre = p.a_rows[mi];
  };
  auto issue = [&](int st, int id) {
    char* sb = smem_c + (st % WS_NST) * WS_STB;
    const bool ok = st * WG_SR + lrow < row_count && id >= 0;
    const uint16_t* sa = A16 + (int64_t)(ok ? id : 0) * p.lda + acol;
    const uint16_t* sd = ok ? D16 + (int64_t)id * p.ldd + dcol : g_zero_row + 8 * (lane & 15);
    const int o = wave * 1024;
    __builtin_amdgcn_global_load_lds((const void*)sa, (lds_void_t*)(sb + o), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(sa + GT), (lds_void_t*)(sb + WG_IMG + o), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)sd, (lds_void_t*)(sb + 2 * WG_IMG + o), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(ok ? sd + GT : sd), (lds_void_t*)(sb + 3 * WG_IMG + o), 16, 0, 0);
  };
  const int gi = lane & 15, q = gi >> 2, pp = gi & 3, g1 = (lane >> 4) & 1;
  int aoff[2][2], doff[4][2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int r = 8 * h + 4 * rd + q;
#pragma unroll
    for (int m = 0; m < 2; ++m)
      aoff[m][rd] = wsw_off(r, (64 * (wk & 1) + 32 * m + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) doff[nb][rd] = wsw_off(r, (32 * nb + 16 * g1) / 8 + (pp >> 1)) + 8 * (pp & 1);
  }
  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  const bool do_bias = p.bslab && tk == 0 && t < 256;
  const int bcp = t & 63, brs = (t >> 6) & 3;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};

  for (int s0 = 0; s0 < WS_NST - 1; ++s0)
    if (s0 < nst) issue(s0, row_id(s0));
  if (IDL) prefetch_block(0);
  for (int st = 0; st < nst; ++st) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (st + WS_NST - 1 <= nst) {
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"((WS_NST - 2) * 4) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const bool blk = IDL && (st % WG_IDB) == 0;
    if (blk) {
      idbuf[((st / WG_IDB) & 1) * WS_IDR + t] = pre;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (blk) prefetch_block(st / WG_IDB + 1);
    if (st + WS_NST - 1 < nst) {
      const int id = IDL ? idbuf[((st / WG_IDB) & 1) * WS_IDR + (st % WG_IDB) * WG_SR + lrow] : row_id(st + WS_NST - 1);
      issue(st + WS_NST - 1, id);
    }
    const char* Sb = smem_c + (st % WS_NST) * WS_STB;
    const char* As = Sb + WG_IMG * (wk >> 1);
    const char* Ds = Sb + WG_IMG * (2 + wn);
    if (do_bias) {
      const char* Db = Sb + WG_IMG * (2 + (bcp >> 5));
      const int bc = 4 * (bcp & 31);
#pragma unroll
      for (int r8 = 0; r8 < WG_SR / 4; ++r8) {
        const int r = (WG_SR / 4) * brs + r8;
        const u32x2 w = *reinterpret_cast<const u32x2*>(Db + wsw_off(r, bc >> 3) + 2 * (bc & 7));
        bs[0] += __uint_as_float(w.x << 16);
        bs[1] += __uint_as_float(w.x & 0xffff0000u);
        bs[2] += __uint_as_float(w.y << 16);
        bs[3] += __uint_as_float(w.y & 0xffff0000u);
      }
    }
#pragma unroll
    for (int t2 = 0; t2 < WG_SR / 16; ++t2) {
      const int po = t2 * 16 * 256;
      u32x4 fa[2], fb[4];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        v4i16 a0 = ds_tr16_nowait(As + po, aoff[m][0]), a1 = ds_tr16_nowait(As + po, aoff[m][1]);
        v4i16 d0 = ds_tr16_nowait(Ds + po, doff[2 * m][0]), d1 = ds_tr16_nowait(Ds + po, doff[2 * m][1]);
        v4i16 e0 = ds_tr16_nowait(Ds + po, doff[2 * m + 1][0]), e1 = ds_tr16_nowait(Ds + po, doff[2 * m + 1][1]);
        tr16_wait(a0, a1, d0, d1);
        asm volatile("" : "+v"(e0), "+v"(e1) :: "memory");
        const u32x2 a0u = __builtin_bit_cast(u32x2, a0), a1u = __builtin_bit_cast(u32x2, a1);
        const u32x2 d0u = __builtin_bit_cast(u32x2, d0), d1u = __builtin_bit_cast(u32x2, d1);
        const u32x2 e0u = __builtin_bit_cast(u32x2, e0), e1u = __builtin_bit_cast(u32x2, e1);
        fa[m] = u32x4{a0u.x, a0u.y, a1u.x, a1u.y};
        fb[2 * m] = u32x4{d0u.x, d0u.y, d1u.x, d1u.y};
        fb[2 * m + 1] = u32x4{e0u.x, e0u.y, e1u.x, e1u.y};
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = mfma_bf16(fa[m], fb[n], acc[m][n]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float* slab = p.slab + (int64_t)c * p.K * p.N;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + 64 * wk + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
      for (int n = 0; n < 4; ++n) slab[(int64_t)k * p.N + n0 + GT * wn + 32 * n + li] = acc[m][n][r];
    }
  if (p.bslab && tk == 0) {                           // fixed-order sum of the 4 row sets per column
    __syncthreads();
    float* bl = reinterpret_cast<float*>(smem_c);     // [4][256]
    if (t < 256) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bl[brs * 2 * GT + 4 * bcp + j] = bs[j];
    }
    __syncthreads();
    if (t < 256) p.bslab[(int64_t)c * p.N + n0 + t] = ((bl[t] + bl[2 * GT + t]) + bl[4 * GT + t]) + bl[6 * GT + t];
  }
}

// Sum the slabs of each group's chunks (chunks of one group are contiguous) into dW[g] (and db).
// Block = 16 float4 columns x 16 chunk lanes; chunk lane c sums chunks c, c+16, ... and the 16
// partials are combined in a fixed order through LDS (deterministic).
// Blocks past the weight columns (wblocks) reduce the bias slab the same way when N % 4 == 0 (the bias
// sums used to be one block per group looping over every chunk: the reduce's long pole).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab,
                                                           const float* __restrict__ bslab,
                                                           const int32_t* __restrict__ gchunk, int K, int N,
                                                           float* dW, int64_t dw_gstride, float* db,
                                                           int64_t db_gstride, int accumulate, int wblocks) {
  __shared__ f32x4 red[16][16];
  const int g = blockIdx.y;
  const int cb = gchunk[2 * g], cn = gchunk[2 * g + 1];
  const bool bias_blk = (int)blockIdx.x >= wblocks;
  const int64_t KN = bias_blk ? (int64_t)N : (int64_t)K * N;     // slab stride per chunk
  const float* src = bias_blk ? bslab : slab;
  float* out = bias_blk ? db + (int64_t)g * db_gstride : dW + (int64_t)g * dw_gstride;
  const int col = threadIdx.x & 15, cl = threadIdx.x >> 4;
  const int64_t i4 = ((int64_t)(bias_blk ? blockIdx.x - wblocks : blockIdx.x) * 16 + col) * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i4 < KN && (!bias_blk || bslab)) {
    int c = cb + cl;
    for (; c + 48 < cb + cn; c += 64) {        // four independent loads in flight per lane
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(src + (int64_t)c * KN + i4);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (int64_t)(c + 16) * KN + i4);
      const f32x4 a2 = *reinterpret_cast<const f32x4*>(src + (int64_t)(c + 32) * KN + i4);
      const f32x4 a3 = *reinterpret_cast<const f32x4*>(src + (int64_t)(c + 48) * KN + i4);
      s += a0; s += a1; s += a2; s += a3;      // fixed order: deterministic
    }
    for (; c < cb + cn; c += 16) s += *reinterpret_cast<const f32x4*>(src + (int64_t)c * KN + i4);
  }
  red[cl][col] = s;
  __syncthreads();
  if (cl == 0 && i4 < KN) {   // a group with no rows (e.g. dedicated groups outside a 1-token tail) -> 0
    f32x4 t = red[0][col];
#pragma unroll
    for (int q = 1; q < 16; ++q) t += red[q][col];
    float* dst = out + i4;
    if (accumulate) t += *reinterpret_cast<const f32x4*>(dst);
    *reinterpret_cast<f32x4*>(dst) = t;
  }
  if (db && N % 4 != 0 && blockIdx.x == 0) {
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
      float t = 0.f;
      if (bslab)
        for (int c = cb; c < cb + cn; ++c) t += bslab[(int64_t)c * N + n];
      float* dst = db + (int64_t)g * db_gstride + n;
      *dst = accumulate ? *dst + t : t;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Transposed weight shadow: dst[g][n][k] = src[g][k][n] for each bank (32x32 LDS tiles).
// banks: [nbanks][6] int64 {src_off, dst_off, G, K, N, first_tile}; tiles of a bank: G*ceil(K/32)*ceil(N/32)
__global__ __launch_bounds__(256) void transpose_banks_kernel(const float* __restrict__ src, float* dst,
                                                              const int64_t* __restrict__ banks, int nbanks) {
  __shared__ float tile[32][33];
  const int64_t tid = blockIdx.x;
  int b = 0;
  while (b + 1 < nbanks && banks[6 * (b + 1) + 5] <= tid) ++b;
  const int64_t* bk = banks + 6 * b;
  const int64_t G = bk[2], K = bk[3], N = bk[4];
  const int64_t tk = (K + 31) / 32, tnn = (N + 31) / 32;
  int64_t rem = tid - bk[5];
  if (rem >= G * tk * tnn) return;
  const int64_t g = rem / (tk * tnn);
  rem %= tk * tnn;
  const int64_t k0 = (rem / tnn) * 32, n0 = (rem % tnn) * 32;
  const float* s = src + bk[0] + g * K * N;
  float* d = dst + bk[1] + g * K * N;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int64_t k = k0 + i, n = n0 + tx;
    tile[i][tx] = (k < K && n < N) ? s[k * N + n] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int64_t n = n0 + i, k = k0 + tx;
    if (k < K && n < N) d[n * K + k] = tile[tx][i];
  }
}

}  // namespace ot

using namespace ot;

extern "C" int ot_transpose_banks(const float* src, float* dst, const int64_t* banks_dev, int nbanks,
                                  int64_t total_tiles, void* stream) {
  OT_REQUIRE(src && dst && banks_dev && nbanks > 0, "ot_transpose_banks: bad args");
  if (total_tiles == 0) return OT_OK;
  hipLaunchKernelGGL(transpose_banks_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, src, dst,
                     banks_dev, nbanks);
  OT_LAUNCH_CHECK("ot_transpose_banks");
  return OT_OK;
}

// process-wide choice of the bf16 weight-gradient tile (ot_wgrad_wide): 0 128 x 128, 1 auto (256 x 256 where K and N
// allow, else 128 x 256), 2 128 x 256, 3 256 x 256
static std::atomic<int> g_wgrad_wide{OT_WGRAD_WIDE};
extern "C" int ot_wgrad_wide(int on) {
  const int prev = g_wgrad_wide.load();
  if (on >= 0) g_wgrad_wide.store(on > 3 ? 3 : on);
  return prev;
}

extern "C" size_t ot_wgrad_workspace_size(int nchunks, int K, int N) {
  return ((size_t)nchunks * K * N + (size_t)nchunks * N) * sizeof(float);
}

static int wgrad_impl(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                      const float* a_rstd, const float* a_gamma,
                      const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                      const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                      float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                      int accumulate, void* workspace, size_t ws_bytes, const float* a_bound, const float* d_bound,
                      int precision, void* stream, const uint32_t* keep = nullptr, int64_t ldkeep = 0,
                      float d_scale = 1.f) {
  OT_REQUIRE(precision == OT_MATMUL_F32 || precision == OT_MATMUL_SPLIT_BF16 || precision == OT_MATMUL_BF16,
             "ot_mixed_gemm_wgrad: unknown precision %d", precision);
  OT_REQUIRE(A && D && dW && chunks && gchunk && workspace, "ot_mixed_gemm_wgrad: null operand");
  OT_REQUIRE(K % 4 == 0 && N % 4 == 0 && lda % 4 == 0 && ldd % 4 == 0 && dw_gstride % 4 == 0,
             "ot_mixed_gemm_wgrad: K, N, lda, ldd, dw_gstride must be multiples of 4");
  OT_REQUIRE(ws_bytes >= ot_wgrad_workspace_size(nchunks, K, N), "ot_mixed_gemm_wgrad: workspace too small");
  const bool dbf = (a_xform & OT_WG_D_BF16) != 0;
  const bool kbits = (a_xform & OT_WG_D_KEEPBITS) != 0;
  a_xform &= ~(OT_WG_D_BF16 | OT_WG_D_KEEPBITS);
  OT_REQUIRE(kbits == (keep != nullptr), "ot_mixed_gemm_wgrad: OT_WG_D_KEEPBITS goes with ot_mixed_gemm_wgrad_keep's keep");
  OT_REQUIRE(!kbits || (precision == OT_MATMUL_SPLIT_BF16 && !dbf && a_xform == OT_AX_GELU && a_bound && d_bound &&
                        N % GT == 0 && ldkeep >= N / 32 && ldkeep % 4 == 0 && ((uintptr_t)keep % 16) == 0),
             "ot_mixed_gemm_wgrad: OT_WG_D_KEEPBITS needs the split mode's pair form (f32 D, OT_AX_GELU, both bounds), "
             "N %% %d == 0, ldkeep >= N / 32, ldkeep %% 4 == 0 and 16-B aligned keep", GT);
  OT_REQUIRE(a_xform != OT_AX_RMSNORM || (a_rstd && a_gamma), "ot_mixed_gemm_wgrad: rmsnorm prologue needs rstd/gamma");
  OT_REQUIRE(!dbf || (precision == OT_MATMUL_BF16 &&
                      (a_xform == OT_AX_NONE || a_xform == OT_AX_RMSNORM || a_xform == OT_AX_BF16) &&
                      ((uintptr_t)D % 8) == 0),
             "ot_mixed_gemm_wgrad: OT_WG_D_BF16 needs the bf16 mode, A form OT_AX_NONE / OT_AX_RMSNORM and 8-B "
             "aligned D rows");
  hipStream_t s = (hipStream_t)stream;
  float* slab = (float*)workspace;
  float* bslab = db ? slab + (size_t)nchunks * K * N : nullptr;
  if (nchunks > 0) {
    WgradArgs p{A, lda, a_rows, a_xform, a_rstd, a_gamma, D, ldd, d_rows, K, N, chunks, nchunks, slab, bslab,
                (int)ceil_div(K, GT), (int)ceil_div(N, GT), a_bound, d_bound, keep, ldkeep, d_scale};
    // the scaled fp16 pair: split mode, f32 operands, D's bound given, and A's (or the RMSNorm prologue's own)
    const bool pair = precision == OT_MATMUL_SPLIT_BF16 && !dbf && d_bound &&
                      ((a_xform == OT_AX_RMSNORM) || ((a_xform == OT_AX_NONE || a_xform == OT_AX_GELU) && a_bound));
    const size_t shmem = (OT_WGRAD_DBUF ? 4 : 2) * WBR * WLD * sizeof(float);
    const bool split = precision != OT_MATMUL_F32;
    OT_REQUIRE(a_xform != OT_AX_BF16 || (precision != OT_MATMUL_F32 && lda % 4 == 0 && ((uintptr_t)A % 8) == 0),
               "ot_mixed_gemm_wgrad: OT_AX_BF16 needs the split / bf16 mode and 8-B aligned rows");
    // both operands bf16 with whole 16-B column chunks: the copy-staged kernel
    const bool copy = dbf && a_xform == OT_AX_BF16 && K % 8 == 0 && N % 8 == 0 && lda % 8 == 0 &&
                      ldd % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)D % 16) == 0 && a_rows == d_rows;
    void (*kern)(WgradArgs) =
        kbits  ? wgrad_split_kernel<OT_AX_GELU, 2, false, true>
        : pair ? (a_xform == OT_AX_NONE      ? wgrad_split_kernel<OT_AX_NONE, 2>
                : a_xform == OT_AX_RMSNORM ? wgrad_split_kernel<OT_AX_RMSNORM, 2>
                                           : wgrad_split_kernel<OT_AX_GELU, 2>)
        : copy ? (a_rows ? wgrad_bf16_kernel<true> : wgrad_bf16_kernel<false>)
        : dbf ? (a_xform == OT_AX_NONE      ? wgrad_split_kernel<OT_AX_NONE, 1, true>
                 : a_xform == OT_AX_BF16    ? wgrad_split_kernel<OT_AX_BF16, 1, true>
                                            : wgrad_split_kernel<OT_AX_RMSNORM, 1, true>)
        : a_xform == OT_AX_BF16 ? (precision == OT_MATMUL_BF16 ? wgrad_split_kernel<OT_AX_BF16, 1>
                                                                : wgrad_split_kernel<OT_AX_BF16, SPLIT_TERMS>)
        : precision == OT_MATMUL_BF16
            ? (a_xform == OT_AX_NONE      ? wgrad_split_kernel<OT_AX_NONE, 1>
               : a_xform == OT_AX_RMSNORM ? wgrad_split_kernel<OT_AX_RMSNORM, 1>
               : a_xform == OT_AX_GELU    ? wgrad_split_kernel<OT_AX_GELU, 1>
                                          : wgrad_split_kernel<-1, 1>)
        : split ? (a_xform == OT_AX_NONE      ? wgrad_split_kernel<OT_AX_NONE, SPLIT_TERMS>
                 : a_xform == OT_AX_RMSNORM ? wgrad_split_kernel<OT_AX_RMSNORM, SPLIT_TERMS>
                 : a_xform == OT_AX_GELU    ? wgrad_split_kernel<OT_AX_GELU, SPLIT_TERMS>
                                            : wgrad_split_kernel<-1, SPLIT_TERMS>)
              : (a_xform == OT_AX_NONE      ? wgrad_kernel<OT_AX_NONE>
                 : a_xform == OT_AX_RMSNORM ? wgrad_kernel<OT_AX_RMSNORM>
                 : a_xform == OT_AX_GELU    ? wgrad_kernel<OT_AX_GELU>
                                            : wgrad_kernel<-1>);
    const size_t split_shmem = 2 * WSOP;
    static std::once_flag lds_once;
    std::call_once(lds_once, [] {
      for (void (*k)(WgradArgs) : {wgrad_kernel<OT_AX_NONE>, wgrad_kernel<OT_AX_RMSNORM>, wgrad_kernel<OT_AX_GELU>,
                                   wgrad_kernel<-1>})
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * WBR * WLD * 4);
      (void)hipGetLastError();
    });
    const size_t copy_shmem = (size_t)WG_LDS;
    if (copy && copy_shmem > 64 * 1024) {
      static std::once_flag copy_once;
      std::call_once(copy_once, [] {
        for (void (*k)(WgradArgs) : {wgrad_bf16_kernel<true>, wgrad_bf16_kernel<false>})
          (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS);
        (void)hipGetLastError();
      });
    }
    const int wgw = g_wgrad_wide.load(std::memory_order_relaxed);
    if (copy && N % (2 * GT) == 0 && K % (2 * GT) == 0 && (wgw == 1 || wgw == 3)) {   // 256 x 256
      static std::once_flag sq_once;
      std::call_once(sq_once, [] {
        for (void (*k)(WgradArgs) : {wgrad_bf16_sq_kernel<true>, wgrad_bf16_sq_kernel<false>})
          (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, WS_LDS);
        (void)hipGetLastError();
      });
      hipLaunchKernelGGL(a_rows ? wgrad_bf16_sq_kernel<true> : wgrad_bf16_sq_kernel<false>,
                         dim3(wgrad_grid(nchunks, (K / (2 * GT)) * (N / (2 * GT)))), dim3(512), (size_t)WS_LDS, s, p);
    } else if (copy && N % (2 * GT) == 0 && wgw) {
      static std::once_flag wide_once;
      std::call_once(wide_once, [] {
        for (void (*k)(WgradArgs) : {wgrad_bf16_wide_kernel<true>, wgrad_bf16_wide_kernel<false>})
          (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, WW_LDS);
        (void)hipGetLastError();
      });
      hipLaunchKernelGGL(a_rows ? wgrad_bf16_wide_kernel<true> : wgrad_bf16_wide_kernel<false>,
                         dim3(wgrad_grid(nchunks, p.ntk * (N / (2 * GT)))), dim3(256), (size_t)WW_LDS, s, p);
    } else {
      hipLaunchKernelGGL(kern, dim3(wgrad_grid(nchunks, p.ntk * p.ntn)), dim3(256),
                         copy ? copy_shmem : split ? split_shmem : shmem, s, p);
    }
    OT_LAUNCH_CHECK("ot_mixed_gemm_wgrad");
  }
  const int wblocks = (int)ceil_div((int64_t)K * N / 4, 16);
  const int bblocks = (db && N % 4 == 0) ? (int)ceil_div((int64_t)N / 4, 16) : 0;
  dim3 rg(wblocks + bblocks, ngroups);
  hipLaunchKernelGGL(wgrad_reduce_kernel, rg, dim3(256), 0, s, slab, bslab, gchunk, K, N, dW, dw_gstride, db,
                     db_gstride, accumulate, wblocks);
  OT_LAUNCH_CHECK("ot_mixed_gemm_wgrad(reduce)");
  return OT_OK;
}

extern "C" int ot_mixed_gemm_wgrad(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                                   const float* a_rstd, const float* a_gamma,
                                   const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                                   const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                                   float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                                   int accumulate, void* workspace, size_t ws_bytes, int precision,
                                   void* stream) {
  return wgrad_impl(A, lda, a_rows, a_xform, a_rstd, a_gamma, D, ldd, d_rows, K, N, chunks, nchunks, gchunk, ngroups,
                    dW, dw_gstride, db, db_gstride, accumulate, workspace, ws_bytes, nullptr, nullptr, precision,
                    stream);
}

extern "C" int ot_mixed_gemm_wgrad_ex(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                                      const float* a_rstd, const float* a_gamma,
                                      const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                                      const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                                      float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                                      int accumulate, void* workspace, size_t ws_bytes, const float* a_bound,
                                      const float* d_bound, int precision, void* stream) {
  return wgrad_impl(A, lda, a_rows, a_xform, a_rstd, a_gamma, D, ldd, d_rows, K, N, chunks, nchunks, gchunk, ngroups,
                    dW, dw_gstride, db, db_gstride, accumulate, workspace, ws_bytes, a_bound, d_bound, precision,
                    stream);
}

extern "C" int ot_mixed_gemm_wgrad_keep(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                                        const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                                        const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                                        float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                                        int accumulate, void* workspace, size_t ws_bytes, const float* a_bound,
                                        const float* d_bound, const uint32_t* keep, int64_t ldkeep, float d_scale,
                                        int precision, void* stream) {
  OT_REQUIRE(keep && (a_xform & OT_WG_D_KEEPBITS), "ot_mixed_gemm_wgrad_keep: needs keep and OT_WG_D_KEEPBITS");
  return wgrad_impl(A, lda, a_rows, a_xform, nullptr, nullptr, D, ldd, d_rows, K, N, chunks, nchunks, gchunk, ngroups,
                    dW, dw_gstride, db, db_gstride, accumulate, workspace, ws_bytes, a_bound, d_bound, precision,
                    stream, keep, ldkeep, d_scale);
}
