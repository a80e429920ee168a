// Group-wise NS tokenizer (paper eq. 6; include/onetrans_hip.h, "group-wise NS tokenizer"): a ragged-K grouped GEMM.
// Every sample row b feeds all G groups; group g reads its own column range [goff[g], goff[g+1]) of the NS matrix A
// and its own rows of the group-major weight bank W [goff[G], d], and writes token g of row b.
//   ot_ns_group_fwd         X[b][g*d + n]     = sum_k A[b][goff[g]+k] W[goff[g]+k][n] + bias[g][n]
//   ot_ns_group_bwd_input   dA[b][goff[g]+k]  = sum_n D[b][g*d + n] W[goff[g]+k][n]
//   ot_ns_group_bwd_weight  dW[goff[g]+k][n] (+)= sum_b A[b][goff[g]+k] D[b][g*d + n],  db[g][n] (+)= sum_b D[b][g*d + n]
//
// Arithmetic: exact f32 on the vector ALU, one fmaf chain per output element in ascending order of the summed
// index (k, n, b): the arithmetic of v_mfma_f32_32x32x2_f32, which issues at the VALU's own f32 peak on gfx950, so
// the matrix core buys no rate here.  The register tiles below hold four consecutive output columns per lane, so
// the forward (bound by its B * G * d * 4-byte output) stores whole 16-byte pieces, 512 contiguous bytes per row and
// half-wave, without a pass through LDS; and a group of any width, K_g = 1 included, runs the same code.
//
// Shapes (256 threads each):
//   fwd     one workgroup per (64-row tile, group, 128-column tile); W_g staged 32 k at a time (a whole [K_g, d] does
//           not fit LDS at d = 512), A staged transposed so a lane reads its 8 rows as two 16-byte pieces.
//   bwd_in  one workgroup per (64-row tile, group, 64-k tile of the group); tiles past the group's K_g leave at once.
//   bwd_w   row chunks x (64-k tile, 64-column tile, group): each chunk writes its partial slab of dW and db, and a
//           second kernel adds the slabs in chunk order (deterministic; no float atomics).
// goff is read on the device only.  A range that leaves [0, goff[G]] or is empty makes its workgroups return before
// they touch memory, so a table that breaks the contract cannot send an access out of bounds.
#include "common.h"

namespace ot {

constexpr int NSG_BM = 64;    // rows of a forward / input-gradient tile
constexpr int NSG_BN = 128;   // columns of a forward tile
constexpr int NSG_KS = 32;    // depth of one LDS stage (k, n or rows)
constexpr int NSG_T = 64;     // the other tile edges (k x n of the weight gradient, k of the input gradient)
constexpr int NSG_PAD = 4;    // transposed stages: row stride 68 floats (16-byte pieces stay aligned)
constexpr int NSG_WG_MAX_CHUNKS = 64;

// group g's range, or false when it is empty or leaves [0, ktot]
__device__ __forceinline__ bool nsg_range(const int32_t* __restrict__ goff, int g, int ktot, int& k0, int& kg) {
  k0 = goff[g];
  const int k1 = goff[g + 1];
  kg = k1 - k0;
  return k0 >= 0 && k1 <= ktot && kg > 0;
}

__global__ __launch_bounds__(256) void ns_group_fwd_kernel(const float* __restrict__ A, int64_t lda,
                                                            const int32_t* __restrict__ goff, int ktot,
                                                            const float* __restrict__ W, const float* __restrict__ bias,
                                                            int B, int d, float* __restrict__ X, int64_t ldx) {
  __shared__ __attribute__((aligned(16))) float As[NSG_KS][NSG_BM + NSG_PAD];   // [k][row]
  __shared__ __attribute__((aligned(16))) float Ws[NSG_KS][NSG_BN];             // [k][n]
  const int g = blockIdx.y;
  int k0, kg;
  if (!nsg_range(goff, g, ktot, k0, kg)) return;
  const int64_t b0 = (int64_t)blockIdx.x * NSG_BM;
  const int n0 = blockIdx.z * NSG_BN;
  const int tid = threadIdx.x;
  const int tx = tid & 31, ty = tid >> 5;          // columns n0 + 4 tx .. + 3, rows b0 + 8 ty .. + 7
  f32x4 acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < kg; ks += NSG_KS) {
    // A stage: 64 rows x 32 k, lanes along k (no alignment assumed: group offsets are arbitrary)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      const int kk = e & 31, r = e >> 5;
      const int64_t b = b0 + r;
      As[kk][r] = (b < B && ks + kk < kg) ? A[b * lda + k0 + ks + kk] : 0.f;
    }
    // W stage: 32 k x 128 columns, 16-byte pieces
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      const int c4 = e & 31, kk = e >> 5;
      const int n = n0 + 4 * c4;
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (ks + kk < kg && n < d) w = *reinterpret_cast<const f32x4*>(W + (int64_t)(k0 + ks + kk) * d + n);
      *reinterpret_cast<f32x4*>(&Ws[kk][4 * c4]) = w;
    }
    __syncthreads();
    const int kend = min(NSG_KS, kg - ks);
    for (int kk = 0; kk < kend; ++kk) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(&Ws[kk][4 * tx]);
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(&As[kk][8 * ty]);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(&As[kk][8 * ty + 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r].x = __builtin_fmaf(a0[r], w.x, acc[r].x);
        acc[r].y = __builtin_fmaf(a0[r], w.y, acc[r].y);
        acc[r].z = __builtin_fmaf(a0[r], w.z, acc[r].z);
        acc[r].w = __builtin_fmaf(a0[r], w.w, acc[r].w);
        acc[r + 4].x = __builtin_fmaf(a1[r], w.x, acc[r + 4].x);
        acc[r + 4].y = __builtin_fmaf(a1[r], w.y, acc[r + 4].y);
        acc[r + 4].z = __builtin_fmaf(a1[r], w.z, acc[r + 4].z);
        acc[r + 4].w = __builtin_fmaf(a1[r], w.w, acc[r + 4].w);
      }
    }
    __syncthreads();
  }
  const int n = n0 + 4 * tx;
  if (n >= d) return;
  const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + (int64_t)g * d + n);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t b = b0 + 8 * ty + r;
    if (b < B) *reinterpret_cast<f32x4*>(X + b * ldx + (int64_t)g * d + n) = acc[r] + bv;
  }
}

__global__ __launch_bounds__(256) void ns_group_bwd_input_kernel(const float* __restrict__ D, int64_t ldd,
                                                                  const int32_t* __restrict__ goff, int ktot,
                                                                  const float* __restrict__ W, int B, int d,
                                                                  float* __restrict__ dA, int64_t lda) {
  __shared__ __attribute__((aligned(16))) float Ds[NSG_KS][NSG_BM + NSG_PAD];   // [n][row]
  __shared__ __attribute__((aligned(16))) float Ws[NSG_KS][NSG_T + NSG_PAD];    // [n][k]
  const int g = blockIdx.y;
  int k0, kg;
  if (!nsg_range(goff, g, ktot, k0, kg)) return;
  const int kt = blockIdx.z * NSG_T;
  if (kt >= kg) return;
  const int64_t b0 = (int64_t)blockIdx.x * NSG_BM;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;          // k kt + 4 tx .. + 3, rows b0 + 4 ty .. + 3
  f32x4 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ns = 0; ns < d; ns += NSG_KS) {
    // D and W stages: 64 rows (samples / k) x 32 n each, read as 16-byte pieces along n, stored transposed
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i;
      const int c4 = e & 7, r = e >> 3;
      const int n = ns + 4 * c4;
      const int64_t b = b0 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
      if (n < d) {
        if (b < B) v = *reinterpret_cast<const f32x4*>(D + b * ldd + (int64_t)g * d + n);
        if (kt + r < kg) w = *reinterpret_cast<const f32x4*>(W + (int64_t)(k0 + kt + r) * d + n);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        Ds[4 * c4 + j][r] = v[j];
        Ws[4 * c4 + j][r] = w[j];
      }
    }
    __syncthreads();
    const int nend = min(NSG_KS, d - ns);
    for (int nn = 0; nn < nend; ++nn) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(&Ws[nn][4 * tx]);
      const f32x4 v = *reinterpret_cast<const f32x4*>(&Ds[nn][4 * ty]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r].x = __builtin_fmaf(v[r], w.x, acc[r].x);
        acc[r].y = __builtin_fmaf(v[r], w.y, acc[r].y);
        acc[r].z = __builtin_fmaf(v[r], w.z, acc[r].z);
        acc[r].w = __builtin_fmaf(v[r], w.w, acc[r].w);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t b = b0 + 4 * ty + r;
    if (b >= B) continue;
    float* dst = dA + b * lda + k0 + kt + 4 * tx;       // (a group may start off a 16-byte line)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (kt + 4 * tx + j < kg) dst[j] = acc[r][j];
  }
}

// chunk c (rows c * chunk_rows ..) of group g: the partial dW tile [64 k][64 n] into slab c, and, from the k-tile 0
// workgroups, the partial db of the tile's columns
__global__ __launch_bounds__(256) void ns_group_wgrad_partial_kernel(const float* __restrict__ A, int64_t lda,
                                                                      const float* __restrict__ D, int64_t ldd,
                                                                      const int32_t* __restrict__ goff, int ktot, int G,
                                                                      int B, int d, int chunk_rows, int ntn,
                                                                      float* __restrict__ slab_w,
                                                                      float* __restrict__ slab_b) {
  __shared__ __attribute__((aligned(16))) float As[NSG_KS][NSG_T];   // [row][k]
  __shared__ __attribute__((aligned(16))) float Ds[NSG_KS][NSG_T];   // [row][n]
  const int g = blockIdx.y, c = blockIdx.z;
  int k0, kg;
  if (!nsg_range(goff, g, ktot, k0, kg)) return;
  const int kt = (blockIdx.x / ntn) * NSG_T;
  const int n0 = (blockIdx.x % ntn) * NSG_T;
  if (kt >= kg) return;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;          // n n0 + 4 tx .. + 3, k kt + 4 ty .. + 3
  const int64_t r0 = (int64_t)c * chunk_rows;
  const int64_t r1 = min<int64_t>(B, r0 + chunk_rows);
  f32x4 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int64_t rs = r0; rs < r1; rs += NSG_KS) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      const int kk = e & 63, r = e >> 6;
      const int64_t b = rs + r;
      As[r][kk] = (b < r1 && kt + kk < kg) ? A[b * lda + k0 + kt + kk] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i;
      const int c4 = e & 15, r = e >> 4;
      const int n = n0 + 4 * c4;
      const int64_t b = rs + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (b < r1 && n < d) v = *reinterpret_cast<const f32x4*>(D + b * ldd + (int64_t)g * d + n);
      *reinterpret_cast<f32x4*>(&Ds[r][4 * c4]) = v;
    }
    __syncthreads();
    const int rend = (int)min<int64_t>(NSG_KS, r1 - rs);
    for (int r = 0; r < rend; ++r) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&Ds[r][4 * tx]);
      const f32x4 a = *reinterpret_cast<const f32x4*>(&As[r][4 * ty]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j].x = __builtin_fmaf(a[j], v.x, acc[j].x);
        acc[j].y = __builtin_fmaf(a[j], v.y, acc[j].y);
        acc[j].z = __builtin_fmaf(a[j], v.z, acc[j].z);
        acc[j].w = __builtin_fmaf(a[j], v.w, acc[j].w);
      }
    }
    if (kt == 0 && tid < NSG_T)
      for (int r = 0; r < rend; ++r) bsum += Ds[r][tid];
    __syncthreads();
  }
  const int n = n0 + 4 * tx;
  if (n < d) {
    float* sw = slab_w + (int64_t)c * ktot * d;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (kt + 4 * ty + j < kg) *reinterpret_cast<f32x4*>(sw + (int64_t)(k0 + kt + 4 * ty + j) * d + n) = acc[j];
  }
  if (kt == 0 && tid < NSG_T && n0 + tid < d) slab_b[((int64_t)c * G + g) * d + n0 + tid] = bsum;
}

// out (+)= the slabs, added in chunk order; elements [0, nw) are dW's, [nw, nw + nb) db's (counts of 16-byte pieces)
__global__ __launch_bounds__(256) void ns_group_wgrad_reduce_kernel(const float* __restrict__ slab_w,
                                                                     const float* __restrict__ slab_b, int64_t nw,
                                                                     int64_t nb, int nchunks, int accumulate,
                                                                     float* __restrict__ dW, float* __restrict__ db) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw + nb) return;
  const bool isw = i < nw;
  const float* src = isw ? slab_w + 4 * i : slab_b + 4 * (i - nw);
  const int64_t stride = 4 * (isw ? nw : nb);
  float* dst = isw ? dW + 4 * i : db + 4 * (i - nw);
  f32x4 s = *reinterpret_cast<const f32x4*>(src);
  for (int c = 1; c < nchunks; ++c) s += *reinterpret_cast<const f32x4*>(src + c * stride);
  if (accumulate) s += *reinterpret_cast<const f32x4*>(dst);
  *reinterpret_cast<f32x4*>(dst) = s;
}

static int nsg_chunk_rows(int B) {
  int cr = 128;
  while (((int64_t)B + cr - 1) / cr > NSG_WG_MAX_CHUNKS) cr *= 2;
  return cr;
}

static inline bool nsg_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the checks every entry point shares
static int nsg_args(const char* who, int B, int G, int ktot, int kmax, int d) {
  OT_REQUIRE(B >= 1, "%s: B=%d must be >= 1", who, B);
  OT_REQUIRE(G >= 1 && G <= 65535, "%s: G=%d must be in [1, 65535]", who, G);
  OT_REQUIRE(d >= 4 && d % 4 == 0 && d <= 512, "%s: d=%d must be a multiple of 4 in [4, 512]", who, d);
  OT_REQUIRE(ktot >= G && ktot <= (1 << 22), "%s: goff[G]=%d must be in [G=%d, 2^22] (every group has a column)", who,
             ktot, G);
  OT_REQUIRE(kmax >= 1 && kmax <= ktot, "%s: kmax=%d must be in [1, goff[G]=%d]", who, kmax, ktot);
  OT_REQUIRE((int64_t)ktot * d < 2147483647LL && (int64_t)G * d < 2147483647LL, "%s: weight bank out of range", who);
  return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" int ot_ns_group_fwd(const float* A, int64_t lda, const int32_t* goff, int G, int ktot, int kmax,
                               const float* W, const float* bias, int B, int d, float* X, int64_t ldx, void* stream) {
  OT_REQUIRE(A && goff && W && bias && X, "ot_ns_group_fwd: null operand");
  OT_TRY(nsg_args("ot_ns_group_fwd", B, G, ktot, kmax, d));
  OT_REQUIRE(lda >= ktot, "ot_ns_group_fwd: lda=%lld is below goff[G]=%d", (long long)lda, ktot);
  OT_REQUIRE(ldx >= (int64_t)G * d && ldx % 4 == 0, "ot_ns_group_fwd: ldx=%lld must be a multiple of 4, >= G*d=%lld",
             (long long)ldx, (long long)G * d);
  OT_REQUIRE(nsg_aligned(W) && nsg_aligned(bias) && nsg_aligned(X), "ot_ns_group_fwd: W, bias and X must be 16-byte aligned");
  hipLaunchKernelGGL(ns_group_fwd_kernel, dim3(ceil_div(B, NSG_BM), G, ceil_div(d, NSG_BN)), dim3(256), 0,
                     (hipStream_t)stream, A, lda, goff, ktot, W, bias, B, d, X, ldx);
  OT_LAUNCH_CHECK("ot_ns_group_fwd");
  return OT_OK;
}

extern "C" int ot_ns_group_bwd_input(const float* D, int64_t ldd, const int32_t* goff, int G, int ktot, int kmax,
                                     const float* W, int B, int d, float* dA, int64_t lda, void* stream) {
  OT_REQUIRE(D && goff && W && dA, "ot_ns_group_bwd_input: null operand");
  OT_TRY(nsg_args("ot_ns_group_bwd_input", B, G, ktot, kmax, d));
  OT_REQUIRE(lda >= ktot, "ot_ns_group_bwd_input: lda=%lld is below goff[G]=%d", (long long)lda, ktot);
  OT_REQUIRE(ldd >= (int64_t)G * d && ldd % 4 == 0,
             "ot_ns_group_bwd_input: ldd=%lld must be a multiple of 4, >= G*d=%lld", (long long)ldd, (long long)G * d);
  OT_REQUIRE(nsg_aligned(W) && nsg_aligned(D), "ot_ns_group_bwd_input: W and D must be 16-byte aligned");
  hipLaunchKernelGGL(ns_group_bwd_input_kernel, dim3(ceil_div(B, NSG_BM), G, ceil_div(kmax, NSG_T)), dim3(256), 0,
                     (hipStream_t)stream, D, ldd, goff, ktot, W, B, d, dA, lda);
  OT_LAUNCH_CHECK("ot_ns_group_bwd_input");
  return OT_OK;
}

extern "C" size_t ot_ns_group_wgrad_workspace_size(int B, int G, int ktot, int d) {
  if (B < 1 || G < 1 || ktot < 1 || d < 1) return 0;
  const int64_t nchunks = ((int64_t)B + nsg_chunk_rows(B) - 1) / nsg_chunk_rows(B);
  return (size_t)(nchunks * ((int64_t)ktot + G) * d) * sizeof(float);
}

extern "C" int ot_ns_group_bwd_weight(const float* A, int64_t lda, const float* D, int64_t ldd, const int32_t* goff,
                                      int G, int ktot, int kmax, int B, int d, float* dW, float* db, int accumulate,
                                      void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(A && D && goff && dW && db, "ot_ns_group_bwd_weight: null operand");
  OT_TRY(nsg_args("ot_ns_group_bwd_weight", B, G, ktot, kmax, d));
  OT_REQUIRE(lda >= ktot, "ot_ns_group_bwd_weight: lda=%lld is below goff[G]=%d", (long long)lda, ktot);
  OT_REQUIRE(ldd >= (int64_t)G * d && ldd % 4 == 0,
             "ot_ns_group_bwd_weight: ldd=%lld must be a multiple of 4, >= G*d=%lld", (long long)ldd, (long long)G * d);
  OT_REQUIRE(nsg_aligned(D) && nsg_aligned(dW) && nsg_aligned(db),
             "ot_ns_group_bwd_weight: D, dW and db must be 16-byte aligned");
  const size_t need = ot_ns_group_wgrad_workspace_size(B, G, ktot, d);
  OT_REQUIRE(workspace && ws_bytes >= need && nsg_aligned(workspace),
             "ot_ns_group_bwd_weight: a 16-byte aligned workspace of %zu bytes is needed, got %zu", need, ws_bytes);
  const int cr = nsg_chunk_rows(B);
  const int nchunks = (int)(((int64_t)B + cr - 1) / cr);
  const int ntn = ceil_div(d, NSG_T);
  float* slab_w = (float*)workspace;
  float* slab_b = slab_w + (int64_t)nchunks * ktot * d;
  hipLaunchKernelGGL(ns_group_wgrad_partial_kernel, dim3(ceil_div(kmax, NSG_T) * ntn, G, nchunks), dim3(256), 0,
                     (hipStream_t)stream, A, lda, D, ldd, goff, ktot, G, B, d, cr, ntn, slab_w, slab_b);
  OT_LAUNCH_CHECK("ot_ns_group_bwd_weight");
  const int64_t nw = (int64_t)ktot * d / 4, nb = (int64_t)G * d / 4;
  hipLaunchKernelGGL(ns_group_wgrad_reduce_kernel, dim3(ceil_div(nw + nb, 256)), dim3(256), 0, (hipStream_t)stream,
                     slab_w, slab_b, nw, nb, nchunks, accumulate, dW, db);
  OT_LAUNCH_CHECK("ot_ns_group_bwd_weight");
  return OT_OK;
}
