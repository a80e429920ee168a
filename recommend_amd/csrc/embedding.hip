// Sparse embedding update (build extension; paper: sparse Adagrad + clip 120,
// rank/scaling_up/oneTrans/translation/complete_translation.md:190).
//
// Keras-2.12 Adagrad on a de-duplicated IndexedSlices gradient:
//   1. (key, position) pairs radix-sorted with rocPRIM (stable => rows of one key stay in
//      position order)
//   2. segment heads + inclusive scan -> unique keys and segment starts
//   3. per unique key: sum of its gradient rows in position order (deterministic)
//   4. clip_by_norm(clip) over the unique-row gradient (one device scalar, no host sync)
//   5. acc[r] += g^2 ; w[r] -= lr * g / sqrt(acc[r] + eps)
// HBM-bound: the row reads in step 3 and the table/accumulator row RMW in step 5.
// Row-wise Adagrad (the *_rowwise entry points) shares steps 1-4 and replaces step 5 by
//   5'. acc[r] += (sum_c g[r, c]^2) / E ; w[r, c] -= lr * g[r, c] / sqrt(acc[r] + eps), acc one float per row
#include "keyed.h"

namespace ot {

__global__ void keys_prep_kernel(const int64_t* __restrict__ keys, int64_t n, int64_t num_rows, uint32_t* k32,
                                 int32_t* vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t k = keys[i];
  k32[i] = (k >= 0 && k < num_rows) ? (uint32_t)k : 0xFFFFFFFFu;   // invalid keys sort last, skipped
  vals[i] = (int32_t)i;
}

__global__ void seg_start_kernel(const int32_t* __restrict__ flags, const int32_t* __restrict__ pos, int64_t n,
                                 int32_t* seg_start, int32_t* nuniq) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) seg_start[pos[i] - 1] = (int32_t)i;
  if (i == n - 1) {
    seg_start[pos[i]] = (int32_t)n;
    nuniq[0] = pos[i];
  }
}

// Hot keys (Zipf) can own tens of thousands of rows: every segment is cut into pieces of at most
// PIECE rows; pass 1 sums each piece, pass 2 sums each key's pieces in order (both deterministic).
constexpr int PIECE = 64;

__global__ void piece_count_kernel(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ nuniq,
                                   int64_t n, int32_t* pcount) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n) return;
  const int U = nuniq[0];
  pcount[s] = s < U ? (seg_start[s + 1] - seg_start[s] + PIECE - 1) / PIECE : 0;
}

// tps = min(E / 4, 64) threads per piece / segment, one float4 each per pass of the column loop (any E % 4 == 0:
// the last pass may be partial).  A 256-thread block holds 256 / tps whole groups; when tps does not divide 256 the
// threads past the last whole group are idle: they must not run on into the next block's first piece / segment.
__global__ __launch_bounds__(256) void piece_sum_kernel(const float* __restrict__ grads, int E,
                                                        const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ seg_start,
                                                        const int32_t* __restrict__ pstart,
                                                        const int32_t* __restrict__ nuniq, int tps, float* psum) {
  const int ppb = 256 / tps;
  const int lp = threadIdx.x / tps;
  const int64_t pc = (int64_t)blockIdx.x * ppb + lp;
  const int lt = threadIdx.x % tps;
  const int U = nuniq[0];
  if (lp >= ppb || pc >= pstart[U]) return;
  const int lo = last_start_le(pstart, U, pc);   // the piece's segment
  const int i0 = seg_start[lo] + (int)(pc - pstart[lo]) * PIECE;
  const int i1 = min(i0 + PIECE, seg_start[lo + 1]);
  for (int c = lt * 4; c < E; c += tps * 4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) acc += *reinterpret_cast<const f32x4*>(grads + (int64_t)perm[i] * E + c);
    *reinterpret_cast<f32x4*>(psum + pc * E + c) = acc;
  }
}

__global__ __launch_bounds__(256) void seg_sum_kernel(const float* __restrict__ psum, int E,
                                                      const uint32_t* __restrict__ ksorted,
                                                      const int32_t* __restrict__ seg_start,
                                                      const int32_t* __restrict__ pstart,
                                                      const int32_t* __restrict__ nuniq, int tps, float* gsum,
                                                      float* sq_part) {
  const int spb = 256 / tps;
  const int ls = threadIdx.x / tps;
  const int64_t s = (int64_t)blockIdx.x * spb + ls;
  const int lt = threadIdx.x % tps;
  float sq = 0.f;
  if (ls < spb && s < nuniq[0] && ksorted[seg_start[s]] != 0xFFFFFFFFu) {
    const int b = pstart[s], e = pstart[s + 1];
    for (int c = lt * 4; c < E; c += tps * 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int q = b; q < e; ++q) acc += *reinterpret_cast<const f32x4*>(psum + (int64_t)q * E + c);
      *reinterpret_cast<f32x4*>(gsum + s * E + c) = acc;
      sq += acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w;
    }
  }
  sq = block_sum_256(sq);
  if (threadIdx.x == 0) sq_part[blockIdx.x] = sq;
}

__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ part, int n, float clip,
                                                         float* scale) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = block_sum_256(s);
  if (threadIdx.x == 0) {
    const float l2 = sqrtf(s);
    scale[0] = clip > 0.f ? clip / fmaxf(l2, clip) : 1.f;
  }
}

__global__ __launch_bounds__(256) void adagrad_apply_kernel(float* table, float* accum, int E,
                                                            const uint32_t* __restrict__ ksorted,
                                                            const int32_t* __restrict__ seg_start,
                                                            const int32_t* __restrict__ nuniq,
                                                            const float* __restrict__ gsum,
                                                            const float* __restrict__ scale, int tps, float lr,
                                                            float eps) {
  const int spb = 256 / tps;
  const int ls = threadIdx.x / tps;
  const int64_t s = (int64_t)blockIdx.x * spb + ls;
  const int lt = threadIdx.x % tps;
  if (ls >= spb || s >= nuniq[0]) return;
  const uint32_t key = ksorted[seg_start[s]];
  if (key == 0xFFFFFFFFu) return;
  const float sc = scale[0];
  float* w = table + (int64_t)key * E;
  float* a = accum + (int64_t)key * E;
  for (int c = lt * 4; c < E; c += tps * 4) {
    f32x4 g = *reinterpret_cast<const f32x4*>(gsum + s * E + c) * sc;
    f32x4 av = *reinterpret_cast<const f32x4*>(a + c) + g * g;
    f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
    wv.x -= lr * g.x / sqrtf(av.x + eps);
    wv.y -= lr * g.y / sqrtf(av.y + eps);
    wv.z -= lr * g.z / sqrtf(av.z + eps);
    wv.w -= lr * g.w / sqrtf(av.w + eps);
    *reinterpret_cast<f32x4*>(a + c) = av;
    *reinterpret_cast<f32x4*>(w + c) = wv;
  }
}

// Dense form of a replicated table's gradient (data-parallel exchange by all-reduce): the unique
// rows' sums scattered into a zeroed [num_rows, E] buffer (unique keys: no conflicts).
__global__ __launch_bounds__(256) void scatter_rows_kernel(float* dense, int E, const uint32_t* __restrict__ ksorted,
                                                           const int32_t* __restrict__ seg_start,
                                                           const int32_t* __restrict__ nuniq,
                                                           const float* __restrict__ gsum, int tps) {
  const int spb = 256 / tps;
  const int ls = threadIdx.x / tps;
  const int64_t s = (int64_t)blockIdx.x * spb + ls;
  const int lt = threadIdx.x % tps;
  if (ls >= spb || s >= nuniq[0]) return;
  const uint32_t key = ksorted[seg_start[s]];
  if (key == 0xFFFFFFFFu) return;
  for (int c = lt * 4; c < E; c += tps * 4)
    *reinterpret_cast<f32x4*>(dense + (int64_t)key * E + c) = *reinterpret_cast<const f32x4*>(gsum + s * E + c);
}

// sum of squares of a dense gradient: per-block partials (fixed grid-stride order: deterministic)
__global__ __launch_bounds__(256) void dense_sumsq_kernel(const float* __restrict__ g, int64_t n4, float* part) {
  float sq = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i);
    sq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  sq = block_sum_256(sq);
  if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

// Keras Adagrad over every row; rows with a zero gradient are left bitwise unchanged (acc + 0,
// w - 0), i.e. exactly the sparse update of the touched rows.
__global__ __launch_bounds__(256) void dense_adagrad_kernel(float* table, float* accum, const float* __restrict__ g,
                                                            int64_t n4, const float* __restrict__ scale, float lr,
                                                            float eps) {
  const float sc = scale[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + 4 * i) * sc;
    if (gv.x == 0.f && gv.y == 0.f && gv.z == 0.f && gv.w == 0.f) continue;
    f32x4 av = *reinterpret_cast<const f32x4*>(accum + 4 * i) + gv * gv;
    f32x4 wv = *reinterpret_cast<const f32x4*>(table + 4 * i);
    wv.x -= lr * gv.x / sqrtf(av.x + eps);
    wv.y -= lr * gv.y / sqrtf(av.y + eps);
    wv.z -= lr * gv.z / sqrtf(av.z + eps);
    wv.w -= lr * gv.w / sqrtf(av.w + eps);
    *reinterpret_cast<f32x4*>(accum + 4 * i) = av;
    *reinterpret_cast<f32x4*>(table + 4 * i) = wv;
  }
}
constexpr int DENSE_GRID = 2048;

// fixed-order sum of the per-block squared-norm partials (one block)
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ part, int n, float* out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = block_sum_256(s);
  if (threadIdx.x == 0) out[0] = s;
}

// clip scale from an externally reduced squared norm (row-sharded tables: sum over owners)
__global__ void clip_from_sumsq_kernel(const float* __restrict__ sumsq, float clip, float* scale) {
  if (threadIdx.x == 0) {
    const float l2 = sqrtf(sumsq[0]);
    scale[0] = clip > 0.f ? clip / fmaxf(l2, clip) : 1.f;
  }
}

// ---- row-wise Adagrad: one accumulator per table row --------------------------------------------------------
//   A[r] += (sum_c g[c]^2) / E ;  W[r, c] -= lr g[c] / sqrt(A[r] + eps)
// A row is worked by tps = tps_for(E) threads, group threadIdx.x / tps of a 256-thread block, as in the kernels
// above; lane lt keeps the row's columns 4 (lt + k tps) .. + 3 of pass k in registers (E <= 1024: at most
// ROW_PASSES passes), so the gradient is read once.
constexpr int ROW_PASSES = 4;

// Sum of squares of one row, the same bits in every thread of the row.  The order is fixed by E alone: a lane adds
// x^2, y^2, z^2, w^2 of its passes in pass order (fmaf chain), the lanes' sums meet in LDS and are added in lane
// order.  No shuffles: when tps is no power of two (E = 12, 20, 24, 40, ...) a row's lanes straddle a wavefront
// boundary.  Every thread of the block calls it (one barrier inside); a thread of no row passes zeros.  The caller
// puts a barrier before the next call (part is read until then).
__device__ __forceinline__ float row_sumsq(const f32x4 (&g)[ROW_PASSES], int tps, float (&part)[256]) {
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_PASSES; ++k) {
    const f32x4 v = g[k];
    q = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, q))));
  }
  part[threadIdx.x] = q;
  __syncthreads();
  const int first = threadIdx.x / tps * tps;
  if (first + tps > 256) return 0.f;              // the threads past the block's last whole group
  float s = 0.f;
  for (int j = 0; j < tps; ++j) s += part[first + j];
  return s;
}

// One row's update by its tps threads (active: this thread has a row; all 256 threads call).  g = the row's
// gradient before the clip scale sc.  The accumulator is read by every lane before row_sumsq's barrier and written
// by lane 0 after it, so no lane can read the new value.  A lane whose four gradients are all zero leaves its
// weights alone, and a row whose sum is zero its accumulator (A + 0 and w - 0 are the same bits): the dense form
// then writes nothing to the rows no key named.
__device__ __forceinline__ void rowwise_update(float* w, float* a, const float* __restrict__ g, int E, float sc,
                                               int tps, int lt, bool active, float lr, float eps,
                                               float (&part)[256]) {
  f32x4 gv[ROW_PASSES];
  float a_old = 0.f;
#pragma unroll
  for (int k = 0; k < ROW_PASSES; ++k) {
    const int c = (lt + k * tps) * 4;
    gv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active && c < E) gv[k] = *reinterpret_cast<const f32x4*>(g + c) * sc;
  }
  if (active) a_old = a[0];
  const float ssq = row_sumsq(gv, tps, part);
  if (!active) return;
  const float a_new = a_old + ssq / (float)E;
  const float den = sqrtf(a_new + eps);
  if (lt == 0 && ssq != 0.f) a[0] = a_new;
#pragma unroll
  for (int k = 0; k < ROW_PASSES; ++k) {
    const int c = (lt + k * tps) * 4;
    const f32x4 v = gv[k];
    if (c >= E || (v.x == 0.f && v.y == 0.f && v.z == 0.f && v.w == 0.f)) continue;
    f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
    wv.x -= lr * v.x / den;
    wv.y -= lr * v.y / den;
    wv.z -= lr * v.z / den;
    wv.w -= lr * v.w / den;
    *reinterpret_cast<f32x4*>(w + c) = wv;
  }
}

__global__ __launch_bounds__(256) void rowwise_apply_kernel(float* table, float* accum_rows, int E,
                                                            const uint32_t* __restrict__ ksorted,
                                                            const int32_t* __restrict__ seg_start,
                                                            const int32_t* __restrict__ nuniq,
                                                            const float* __restrict__ gsum,
                                                            const float* __restrict__ scale, int tps, float lr,
                                                            float eps) {
  __shared__ float part[256];
  const int spb = 256 / tps;
  const int ls = threadIdx.x / tps;
  const int64_t s = (int64_t)blockIdx.x * spb + ls;
  const int lt = threadIdx.x % tps;
  uint32_t key = 0xFFFFFFFFu;
  if (ls < spb && s < nuniq[0]) key = ksorted[seg_start[s]];
  const bool active = key != 0xFFFFFFFFu;
  const int64_t r = active ? (int64_t)key : 0, sr = active ? s : 0;
  rowwise_update(table + r * E, accum_rows + r, gsum + sr * E, E, scale[0], tps, lt, active, lr, eps, part);
}

// The dense form: every row of the table against the all-reduced [num_rows, E] gradient, 256 / tps rows per block
// and pass of the grid-stride loop (the same row-to-threads mapping as above, hence the same bits).
__global__ __launch_bounds__(256) void dense_rowwise_kernel(float* table, float* accum_rows,
                                                            const float* __restrict__ g, int64_t num_rows, int E,
                                                            const float* __restrict__ scale, int tps, float lr,
                                                            float eps) {
  __shared__ float part[256];
  const int rpb = 256 / tps;
  const int ls = threadIdx.x / tps;
  const int lt = threadIdx.x % tps;
  const float sc = scale[0];
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < num_rows; base += (int64_t)gridDim.x * rpb) {
    const bool active = ls < rpb && base + ls < num_rows;
    const int64_t r = active ? base + ls : 0;
    rowwise_update(table + r * E, accum_rows + r, g + r * E, E, sc, tps, lt, active, lr, eps, part);
    __syncthreads();                               // part is written again in the next pass
  }
}

struct SparseWs {
  uint32_t *k_in, *k_out;
  int32_t *v_in, *v_out, *flags, *pos, *seg_start, *nuniq, *pcount, *pstart;
  float *gsum, *psum, *sq_part, *scale;
  void* tmp;
  size_t tmp_bytes, total;
};

inline int tps_for(int E) {
  int t = E / 4;
  return t > 64 ? 64 : t;
}

SparseWs carve(void* base, int64_t n, int E) {
  SparseWs w{};
  w.tmp_bytes = std::max({sort_pairs_bytes<uint32_t>(n, 32), inclusive_scan_bytes<int32_t>(n),
                          exclusive_scan_bytes<int32_t>(n + 1)});
  const int spb = 256 / tps_for(E);
  const int64_t nblk = (n + spb - 1) / spb;
  Carver c(base);
  w.k_in = c.take<uint32_t>(n); w.k_out = c.take<uint32_t>(n);
  w.v_in = c.take<int32_t>(n); w.v_out = c.take<int32_t>(n);
  w.flags = c.take<int32_t>(n); w.pos = c.take<int32_t>(n);
  w.seg_start = c.take<int32_t>(n + 1); w.nuniq = c.take<int32_t>(1);
  w.pcount = c.take<int32_t>(n + 1); w.pstart = c.take<int32_t>(n + 1);
  w.gsum = c.take<float>((size_t)n * E); w.psum = c.take<float>((size_t)(n + n / PIECE + 1) * E);
  w.sq_part = c.take<float>(nblk); w.scale = c.take<float>(1);
  w.tmp = c.take<char>(w.tmp_bytes);
  w.total = c.total();
  return w;
}

}  // namespace ot

using namespace ot;

extern "C" size_t ot_sparse_adagrad_workspace_size(int64_t n, int E) {
  if (n <= 0) return 256;
  return carve(nullptr, n, E).total;
}

// steps 1-3 (+ the per-block squared-norm partials of the unique-row sums): fills w.k_out,
// w.seg_start, w.nuniq, w.gsum, w.sq_part
static int segment_rows(SparseWs& w, int E, int64_t num_rows, const int64_t* keys, const float* grads,
                        int64_t n, hipStream_t s) {
  const unsigned g1 = ceil_div(n, 256);
  hipLaunchKernelGGL(keys_prep_kernel, dim3(g1), dim3(256), 0, s, keys, n, num_rows, w.k_in, w.v_in);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(prep)");
  int end_bit = 1;
  while (end_bit < 32 && ((uint64_t)1 << end_bit) < (uint64_t)num_rows + 1) ++end_bit;
  // 2^end_bit > num_rows: the invalid sentinel's low bits (2^end_bit - 1) still sort after every valid key
  OT_TRY(sort_pairs(w.tmp, w.tmp_bytes, w.k_in, w.k_out, w.v_in, w.v_out, n, end_bit, s, "ot_sparse_adagrad(sort)"));
  OT_TRY(run_index(w.k_out, n, w.flags, w.pos, w.tmp, w.tmp_bytes, s, "ot_sparse_adagrad(flags)",
                   "ot_sparse_adagrad(scan)"));
  hipLaunchKernelGGL(seg_start_kernel, dim3(g1), dim3(256), 0, s, w.flags, w.pos, n, w.seg_start, w.nuniq);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(segments)");
  const int tps = tps_for(E);
  hipLaunchKernelGGL(piece_count_kernel, dim3(ceil_div(n + 1, 256)), dim3(256), 0, s, w.seg_start, w.nuniq, n,
                     w.pcount);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(pieces)");
  OT_TRY(exclusive_scan(w.tmp, w.tmp_bytes, w.pcount, w.pstart, n + 1, s, "ot_sparse_adagrad(piece scan)"));
  const unsigned gp = ceil_div(n + n / PIECE + 1, 256 / tps);
  hipLaunchKernelGGL(piece_sum_kernel, dim3(gp), dim3(256), 0, s, grads, E, w.v_out, w.seg_start, w.pstart, w.nuniq,
                     tps, w.psum);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(piecesum)");
  const unsigned g2 = ceil_div(n, 256 / tps);
  hipLaunchKernelGGL(seg_sum_kernel, dim3(g2), dim3(256), 0, s, w.psum, E, w.k_out, w.seg_start, w.pstart, w.nuniq,
                     tps, w.gsum, w.sq_part);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(segsum)");
  return OT_OK;
}

extern "C" int ot_sparse_adagrad(float* table, float* accum, int E, int64_t num_rows, const int64_t* keys,
                                 const float* grads, int64_t n, float lr, float eps, float clip, void* workspace,
                                 size_t ws_bytes, void* stream) {
  OT_REQUIRE(table && accum && keys && grads, "ot_sparse_adagrad: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0 && E <= 1024, "ot_sparse_adagrad: E=%d must be a multiple of 4 <= 1024", E);
  OT_REQUIRE(num_rows > 0 && num_rows < 0xFFFFFFFFLL, "ot_sparse_adagrad: num_rows out of range");
  OT_REQUIRE(n >= 0 && n < 2147483647LL, "ot_sparse_adagrad: n out of range");
  if (n == 0) return OT_OK;
  SparseWs w = carve(workspace, n, E);
  OT_REQUIRE(ws_bytes >= w.total, "ot_sparse_adagrad: workspace too small (%zu < %zu)", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  OT_TRY(segment_rows(w, E, num_rows, keys, grads, n, s));
  const int tps = tps_for(E);
  const unsigned g2 = ceil_div(n, 256 / tps);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, s, w.sq_part, (int)g2, clip, w.scale);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(clip)");
  hipLaunchKernelGGL(adagrad_apply_kernel, dim3(g2), dim3(256), 0, s, table, accum, E, w.k_out, w.seg_start, w.nuniq,
                     w.gsum, w.scale, tps, lr, eps);
  OT_LAUNCH_CHECK("ot_sparse_adagrad(apply)");
  return OT_OK;
}

extern "C" int ot_sparse_grad_dense(int E, int64_t num_rows, const int64_t* keys, const float* grads, int64_t n,
                                    float* dense, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(keys && grads && dense, "ot_sparse_grad_dense: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0 && E <= 1024, "ot_sparse_grad_dense: E=%d must be a multiple of 4 <= 1024", E);
  OT_REQUIRE(num_rows > 0 && num_rows < 0xFFFFFFFFLL, "ot_sparse_grad_dense: num_rows out of range");
  OT_REQUIRE(n >= 0 && n < 2147483647LL, "ot_sparse_grad_dense: n out of range");
  if (n == 0) return OT_OK;
  SparseWs w = carve(workspace, n, E);
  OT_REQUIRE(ws_bytes >= w.total, "ot_sparse_grad_dense: workspace too small (%zu < %zu)", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  OT_TRY(segment_rows(w, E, num_rows, keys, grads, n, s));
  const int tps = tps_for(E);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(ceil_div(n, 256 / tps)), dim3(256), 0, s, dense, E, w.k_out,
                     w.seg_start, w.nuniq, w.gsum, tps);
  OT_LAUNCH_CHECK("ot_sparse_grad_dense(scatter)");
  return OT_OK;
}

extern "C" size_t ot_dense_adagrad_workspace_size(void) { return (DENSE_GRID + 64) * sizeof(float); }

extern "C" int ot_dense_adagrad(float* table, float* accum, const float* grad, int64_t num_rows, int E, float lr,
                                float eps, float clip, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(table && accum && grad && workspace, "ot_dense_adagrad: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0, "ot_dense_adagrad: E must be a multiple of 4");
  OT_REQUIRE(ws_bytes >= ot_dense_adagrad_workspace_size(), "ot_dense_adagrad: workspace too small");
  if (num_rows <= 0) return OT_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n4 = num_rows * E / 4;
  float* part = (float*)workspace;
  float* scale = part + DENSE_GRID;
  hipLaunchKernelGGL(dense_sumsq_kernel, dim3(DENSE_GRID), dim3(256), 0, s, grad, n4, part);
  OT_LAUNCH_CHECK("ot_dense_adagrad(norm)");
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, s, part, DENSE_GRID, clip, scale);
  OT_LAUNCH_CHECK("ot_dense_adagrad(clip)");
  hipLaunchKernelGGL(dense_adagrad_kernel, dim3(DENSE_GRID), dim3(256), 0, s, table, accum, grad, n4, scale, lr, eps);
  OT_LAUNCH_CHECK("ot_dense_adagrad(apply)");
  return OT_OK;
}

// Two-phase form for row-sharded tables, whose clip_by_norm spans every owner's rows: prepare
// de-duplicates this rank's received (key, row) pairs and writes the local squared norm; the caller
// all-reduces it; finish applies clip + Adagrad with the global norm.  The workspace (size
// ot_sparse_adagrad_workspace_size(n, E)) carries the segmentation from prepare to finish.
extern "C" int ot_sparse_prepare(int E, int64_t num_rows, const int64_t* keys, const float* grads, int64_t n,
                                 float* sumsq_out, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(keys && grads && sumsq_out && workspace, "ot_sparse_prepare: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0 && E <= 1024, "ot_sparse_prepare: E=%d must be a multiple of 4 <= 1024", E);
  OT_REQUIRE(num_rows > 0 && num_rows < 0xFFFFFFFFLL, "ot_sparse_prepare: num_rows out of range");
  OT_REQUIRE(n >= 0 && n < 2147483647LL, "ot_sparse_prepare: n out of range");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    (void)hipMemsetAsync(sumsq_out, 0, sizeof(float), s);
    return OT_OK;
  }
  SparseWs w = carve(workspace, n, E);
  OT_REQUIRE(ws_bytes >= w.total, "ot_sparse_prepare: workspace too small (%zu < %zu)", ws_bytes, w.total);
  OT_TRY(segment_rows(w, E, num_rows, keys, grads, n, s));
  const unsigned g2 = ceil_div(n, 256 / tps_for(E));
  hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, s, w.sq_part, (int)g2, sumsq_out);
  OT_LAUNCH_CHECK("ot_sparse_prepare(sumsq)");
  return OT_OK;
}

extern "C" int ot_sparse_finish(float* table, float* accum, int E, int64_t n, float lr, float eps, float clip,
                                const float* sumsq_total, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(table && accum && sumsq_total && workspace, "ot_sparse_finish: null operand");
  if (n <= 0) return OT_OK;
  SparseWs w = carve(workspace, n, E);
  OT_REQUIRE(ws_bytes >= w.total, "ot_sparse_finish: workspace too small (%zu < %zu)", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_from_sumsq_kernel, dim3(1), dim3(64), 0, s, sumsq_total, clip, w.scale);
  OT_LAUNCH_CHECK("ot_sparse_finish(clip)");
  const int tps = tps_for(E);
  const unsigned g2 = ceil_div(n, 256 / tps);
  hipLaunchKernelGGL(adagrad_apply_kernel, dim3(g2), dim3(256), 0, s, table, accum, E, w.k_out, w.seg_start, w.nuniq,
                     w.gsum, w.scale, tps, lr, eps);
  OT_LAUNCH_CHECK("ot_sparse_finish(apply)");
  return OT_OK;
}

// ---- row-wise Adagrad entry points: the three forms above with one accumulator per table row ----------------
static int launch_rowwise_apply(const SparseWs& w, float* table, float* accum_rows, int E, int64_t n, float lr,
                                float eps, hipStream_t s, const char* label) {
  const int tps = tps_for(E);
  hipLaunchKernelGGL(rowwise_apply_kernel, dim3(ceil_div(n, 256 / tps)), dim3(256), 0, s, table, accum_rows, E,
                     w.k_out, w.seg_start, w.nuniq, w.gsum, w.scale, tps, lr, eps);
  OT_LAUNCH_CHECK(label);
  return OT_OK;
}

extern "C" int ot_sparse_adagrad_rowwise(float* table, float* accum_rows, int E, int64_t num_rows,
                                         const int64_t* keys, const float* grads, int64_t n, float lr, float eps,
                                         float clip, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(table && accum_rows && keys && grads, "ot_sparse_adagrad_rowwise: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0 && E <= 1024, "ot_sparse_adagrad_rowwise: E=%d must be a multiple of 4 <= 1024", E);
  OT_REQUIRE(num_rows > 0 && num_rows < 0xFFFFFFFFLL, "ot_sparse_adagrad_rowwise: num_rows out of range");
  OT_REQUIRE(n >= 0 && n < 2147483647LL, "ot_sparse_adagrad_rowwise: n out of range");
  if (n == 0) return OT_OK;
  SparseWs w = carve(workspace, n, E);
  OT_REQUIRE(ws_bytes >= w.total, "ot_sparse_adagrad_rowwise: workspace too small (%zu < %zu)", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  OT_TRY(segment_rows(w, E, num_rows, keys, grads, n, s));
  const unsigned g2 = ceil_div(n, 256 / tps_for(E));
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, s, w.sq_part, (int)g2, clip, w.scale);
  OT_LAUNCH_CHECK("ot_sparse_adagrad_rowwise(clip)");
  return launch_rowwise_apply(w, table, accum_rows, E, n, lr, eps, s, "ot_sparse_adagrad_rowwise(apply)");
}

extern "C" int ot_dense_adagrad_rowwise(float* table, float* accum_rows, const float* grad, int64_t num_rows, int E,
                                        float lr, float eps, float clip, void* workspace, size_t ws_bytes,
                                        void* stream) {
  OT_REQUIRE(table && accum_rows && grad && workspace, "ot_dense_adagrad_rowwise: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0 && E <= 1024, "ot_dense_adagrad_rowwise: E=%d must be a multiple of 4 <= 1024", E);
  OT_REQUIRE(ws_bytes >= ot_dense_adagrad_workspace_size(), "ot_dense_adagrad_rowwise: workspace too small");
  if (num_rows <= 0) return OT_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n4 = num_rows * E / 4;
  float* part = (float*)workspace;
  float* scale = part + DENSE_GRID;
  hipLaunchKernelGGL(dense_sumsq_kernel, dim3(DENSE_GRID), dim3(256), 0, s, grad, n4, part);
  OT_LAUNCH_CHECK("ot_dense_adagrad_rowwise(norm)");
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, s, part, DENSE_GRID, clip, scale);
  OT_LAUNCH_CHECK("ot_dense_adagrad_rowwise(clip)");
  const int tps = tps_for(E);
  const unsigned grid = std::min<int64_t>(DENSE_GRID, ceil_div(num_rows, 256 / tps));
  hipLaunchKernelGGL(dense_rowwise_kernel, dim3(grid), dim3(256), 0, s, table, accum_rows, grad, num_rows, E, scale,
                     tps, lr, eps);
  OT_LAUNCH_CHECK("ot_dense_adagrad_rowwise(apply)");
  return OT_OK;
}

extern "C" int ot_sparse_finish_rowwise(float* table, float* accum_rows, int E, int64_t n, float lr, float eps,
                                        float clip, const float* sumsq_total, void* workspace, size_t ws_bytes,
                                        void* stream) {
  OT_REQUIRE(table && accum_rows && sumsq_total && workspace, "ot_sparse_finish_rowwise: null operand");
  OT_REQUIRE(E > 0 && E % 4 == 0 && E <= 1024, "ot_sparse_finish_rowwise: E=%d must be a multiple of 4 <= 1024", E);
  if (n <= 0) return OT_OK;
  SparseWs w = carve(workspace, n, E);
  OT_REQUIRE(ws_bytes >= w.total, "ot_sparse_finish_rowwise: workspace too small (%zu < %zu)", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_from_sumsq_kernel, dim3(1), dim3(64), 0, s, sumsq_total, clip, w.scale);
  OT_LAUNCH_CHECK("ot_sparse_finish_rowwise(clip)");
  return launch_rowwise_apply(w, table, accum_rows, E, n, lr, eps, s, "ot_sparse_finish_rowwise(apply)");
}
