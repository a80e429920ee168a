// Streaming evaluation metrics (include/onetrans_hip.h, "streaming metrics"): the per-step metric update of
// the reference trainer (train.py:140-150, 176-185; evaluate.py:91-104) as one stream-ordered launch.
//   ot_metrics_update   per task: a histogram of the probabilities over caller-given thresholds, split by label
//                       class, and the running sums behind MSE / MAE / logloss
// The state is additive: counts are exact integers (64-bit integer atomics commute), the double sums are
// reduced in a fixed order (thread -> wave -> workgroup -> workgroups in index order, no float atomics), so a
// state is bit-reproducible from run to run.  Everything a metric reports (AUC, accuracy, precision, recall,
// F1, ...) is finalised on the host from this state (recommend_amd/metrics.py).
#include "common.h"

namespace ot {

constexpr int METRICS_MAX_NB = 1024;     // thresholds
constexpr int METRICS_QUAD_ELEMS = 1024; // samples per workgroup pass: 256 threads x 4
constexpr int METRICS_MAX_BLOCKS = 128;  // workgroups per task (the rest is grid-strided)

inline int metrics_blocks(int B) {
  const int64_t b = ((int64_t)B + METRICS_QUAD_ELEMS - 1) / METRICS_QUAD_ELEMS;
  return (int)(b < 1 ? 1 : (b > METRICS_MAX_BLOCKS ? METRICS_MAX_BLOCKS : b));
}

// One sample of task t: its bin and its terms.  bin = #{j : (double)p > bounds[j]} (bounds ascending, so the
// count is the first j with !(bounds[j] < p); every compare with a NaN is false: bin 0).
struct MetricAcc {
  double se, ae, bce;
};
__device__ __forceinline__ void metrics_sample(float pf, float yf, const double* sb, int nb, unsigned* hist,
                                               MetricAcc& a) {
  const double p = (double)pf, y = (double)yf;
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  atomicAdd(&hist[(yf > 0.5f ? nb + 1 : 0) + lo], 1u);
  const double d = p - y;
  a.se += d * d;
  a.ae += fabs(d);
  // oracle.keras_math.keras_bce on the probability (explicit compares: a NaN stays a NaN, as in np.clip)
  const double eps = 1e-7;
  const double pc = p < eps ? eps : (p > 1.0 - eps ? 1.0 - eps : p);
  a.bce += -(y * log(pc + eps) + (1.0 - y) * log(1.0 - pc + eps));
}

// grid (metrics_blocks(B), T), 256 threads.  Thread i of workgroup g takes the quads (4 consecutive samples)
// g*256 + i, + gridDim.x*256, ...: the same samples in the same order whether they are loaded as one 16-byte
// vector (VEC: both task rows 16-byte aligned) or as guarded scalars, so the sums do not depend on alignment.
// part[(t*gridDim.x + g)*3 + {0,1,2}] = this workgroup's {sum (p-y)^2, sum |p-y|, sum bce}.
template <bool VEC>
__global__ __launch_bounds__(256) void metrics_update_kernel(const float* __restrict__ probs,
                                                             const float* __restrict__ labels, int B,
                                                             int64_t task_stride, const double* __restrict__ bounds,
                                                             int nb, unsigned long long* counts, double* part) {
  __shared__ double sb[METRICS_MAX_NB];
  __shared__ unsigned hist[2 * (METRICS_MAX_NB + 1)];
  __shared__ double red[4][3];
  const int t = blockIdx.y, tid = threadIdx.x;
  const int nh = 2 * (nb + 1);
  for (int i = tid; i < nb; i += 256) sb[i] = bounds[i];
  for (int i = tid; i < nh; i += 256) hist[i] = 0u;
  __syncthreads();
  const float* p = probs + (int64_t)t * task_stride;
  const float* y = labels + (int64_t)t * task_stride;
  const int64_t nquad = ((int64_t)B + 3) >> 2;
  MetricAcc a = {0.0, 0.0, 0.0};
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int64_t i0 = q << 2;
    if (VEC && i0 + 3 < B) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(y + i0);
#pragma unroll
      for (int k = 0; k < 4; ++k) metrics_sample(pv[k], yv[k], sb, nb, hist, a);
    } else {
      for (int k = 0; k < 4; ++k)
        if (i0 + k < B) metrics_sample(p[i0 + k], y[i0 + k], sb, nb, hist, a);
    }
  }
  a.se = wave_sum(a.se);
  a.ae = wave_sum(a.ae);
  a.bce = wave_sum(a.bce);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = a.se;
    red[tid >> 6][1] = a.ae;
    red[tid >> 6][2] = a.bce;
  }
  __syncthreads();
  if (tid < 3) part[((int64_t)t * gridDim.x + blockIdx.x) * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  // only the bins this workgroup touched go to memory (an AUC histogram of one batch is mostly empty)
  unsigned long long* c = counts + (int64_t)t * nh;
  for (int i = tid; i < nh; i += 256) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&c[i], (unsigned long long)v);
  }
}

// grid T, 64 threads: sums[t] += {B, the workgroups' partials folded in index order}
__global__ void metrics_fold_kernel(const double* __restrict__ part, int nblk, int B, double* sums) {
  const int t = blockIdx.x, k = threadIdx.x;
  if (k == 0) sums[t * 4] += (double)B;
  if (k >= 1 && k <= 3) {
    double s = 0.0;
    for (int g = 0; g < nblk; ++g) s += part[((int64_t)t * nblk + g) * 3 + (k - 1)];
    sums[t * 4 + k] += s;
  }
}

// ---- the weighted sibling (ot_metrics_update_weighted) ----
// A weight is clamped to [0, 2^16] (NaN and negatives: 0) and rounded to the nearest multiple of 2^-24 (ties to
// even): the count of such units, an integer <= 2^40.  The histogram and sum w are integers in those units, so the
// state stays exact and commutative.
__device__ __forceinline__ unsigned long long metrics_weight_units(float w) {
  const float c = w > 0.f ? fminf(w, 65536.f) : 0.f;
  return (unsigned long long)__double2ll_rn((double)c * (double)OT_METRICS_WEIGHT_ONE);
}

// metrics_sample under a weight of u units: nothing at all for u == 0 (the entry is skipped, whatever it holds)
__device__ __forceinline__ void metrics_sample_weighted(float pf, float yf, unsigned long long u, const double* sb,
                                                        int nb, unsigned long long* hist, MetricAcc& a,
                                                        unsigned long long& wsum) {
  if (u == 0ull) return;
  const double p = (double)pf, y = (double)yf, w = (double)u;
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  atomicAdd(&hist[(yf > 0.5f ? nb + 1 : 0) + lo], u);
  wsum += u;
  const double d = p - y;
  a.se += w * (d * d);
  a.ae += w * fabs(d);
  const double eps = 1e-7;
  const double pc = p < eps ? eps : (p > 1.0 - eps ? 1.0 - eps : p);
  a.bce += w * -(y * log(pc + eps) + (1.0 - y) * log(1.0 - pc + eps));
}

// The quad walk of metrics_update_kernel with a third operand: task t's weights at weights + t * weight_stride
// (stride 0: one row for every task).  part as above; wpart[t*gridDim.x + g] = this workgroup's sum of units.
template <bool VEC>
__global__ __launch_bounds__(256) void metrics_update_weighted_kernel(
    const float* __restrict__ probs, const float* __restrict__ labels, const float* __restrict__ weights, int B,
    int64_t task_stride, int64_t weight_stride, const double* __restrict__ bounds, int nb, unsigned long long* counts,
    double* part, unsigned long long* wpart) {
  __shared__ double sb[METRICS_MAX_NB];
  __shared__ unsigned long long hist[2 * (METRICS_MAX_NB + 1)];
  __shared__ double red[4][3];
  __shared__ unsigned long long wtot;
  const int t = blockIdx.y, tid = threadIdx.x;
  const int nh = 2 * (nb + 1);
  for (int i = tid; i < nb; i += 256) sb[i] = bounds[i];
  for (int i = tid; i < nh; i += 256) hist[i] = 0ull;
  if (tid == 0) wtot = 0ull;
  __syncthreads();
  const float* p = probs + (int64_t)t * task_stride;
  const float* y = labels + (int64_t)t * task_stride;
  const float* w = weights + (int64_t)t * weight_stride;
  const int64_t nquad = ((int64_t)B + 3) >> 2;
  MetricAcc a = {0.0, 0.0, 0.0};
  unsigned long long wsum = 0ull;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int64_t i0 = q << 2;
    if (VEC && i0 + 3 < B) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(y + i0);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + i0);
#pragma unroll
      for (int k = 0; k < 4; ++k) metrics_sample_weighted(pv[k], yv[k], metrics_weight_units(wv[k]), sb, nb, hist, a, wsum);
    } else {
      for (int k = 0; k < 4; ++k)
        if (i0 + k < B)
          metrics_sample_weighted(p[i0 + k], y[i0 + k], metrics_weight_units(w[i0 + k]), sb, nb, hist, a, wsum);
    }
  }
  if (wsum) atomicAdd(&wtot, wsum);            // integer: exact in any order
  a.se = wave_sum(a.se);
  a.ae = wave_sum(a.ae);
  a.bce = wave_sum(a.bce);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = a.se;
    red[tid >> 6][1] = a.ae;
    red[tid >> 6][2] = a.bce;
  }
  __syncthreads();
  const int64_t slot = (int64_t)t * gridDim.x + blockIdx.x;
  if (tid < 3) part[slot * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  if (tid == 3) wpart[slot] = wtot;
  unsigned long long* c = counts + (int64_t)t * nh;
  for (int i = tid; i < nh; i += 256) {
    const unsigned long long v = hist[i];
    if (v) atomicAdd(&c[i], v);
  }
}

// grid T, 64 threads: sums[t] += {the workgroups' units added as integers, the partials folded in index order}
__global__ void metrics_fold_weighted_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ wpart,
                                             int nblk, double* sums) {
  const int t = blockIdx.x, k = threadIdx.x;
  if (k == 0) {
    unsigned long long s = 0ull;
    for (int g = 0; g < nblk; ++g) s += wpart[(int64_t)t * nblk + g];
    sums[t * 4] += (double)s;
  }
  if (k >= 1 && k <= 3) {
    double s = 0.0;
    for (int g = 0; g < nblk; ++g) s += part[((int64_t)t * nblk + g) * 3 + (k - 1)];
    sums[t * 4 + k] += s;
  }
}

}  // namespace ot

using namespace ot;

extern "C" size_t ot_metrics_workspace_size(int T, int B) {
  if (T < 1 || B < 1) return 0;
  return (size_t)T * metrics_blocks(B) * 3 * sizeof(double);
}

extern "C" int ot_metrics_update(const float* probs, const float* labels, int T, int B, int64_t task_stride,
                                 const double* bounds, int nb, int64_t* counts, double* sums, void* workspace,
                                 size_t ws_bytes, void* stream) {
  OT_REQUIRE(probs && labels && bounds && counts && sums && workspace, "ot_metrics_update: null operand");
  OT_REQUIRE(T > 0 && T <= 32, "ot_metrics_update: 1..32 tasks");
  OT_REQUIRE(nb > 0 && nb <= METRICS_MAX_NB, "ot_metrics_update: 1..%d thresholds", METRICS_MAX_NB);
  OT_REQUIRE(B > 0, "ot_metrics_update: empty batch");
  OT_REQUIRE(task_stride >= B, "ot_metrics_update: task_stride < B");
  OT_REQUIRE(ws_bytes >= ot_metrics_workspace_size(T, B), "ot_metrics_update: workspace too small");
  OT_REQUIRE((reinterpret_cast<uintptr_t>(probs) & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(bounds) & 7) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(sums) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "ot_metrics_update: misaligned operand");
  const int nblk = metrics_blocks(B);
  const bool vec = ((reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(labels)) & 15) == 0 &&
                   (T == 1 || (task_stride & 3) == 0);
  auto kern = vec ? metrics_update_kernel<true> : metrics_update_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(nblk, T), dim3(256), 0, (hipStream_t)stream, probs, labels, B, task_stride, bounds, nb,
                     reinterpret_cast<unsigned long long*>(counts), (double*)workspace);
  OT_LAUNCH_CHECK("ot_metrics_update");
  hipLaunchKernelGGL(metrics_fold_kernel, dim3(T), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, nblk, B,
                     sums);
  OT_LAUNCH_CHECK("ot_metrics_update(fold)");
  return OT_OK;
}

extern "C" size_t ot_metrics_weighted_workspace_size(int T, int B) {
  if (T < 1 || B < 1) return 0;
  return (size_t)T * metrics_blocks(B) * (3 * sizeof(double) + sizeof(unsigned long long));
}

extern "C" int ot_metrics_update_weighted(const float* probs, const float* labels, const float* weights, int T, int B,
                                          int64_t task_stride, int64_t weight_stride, const double* bounds, int nb,
                                          int64_t* counts, double* sums, void* workspace, size_t ws_bytes,
                                          void* stream) {
  OT_REQUIRE(probs && labels && weights && bounds && counts && sums && workspace,
             "ot_metrics_update_weighted: null operand");
  OT_REQUIRE(T > 0 && T <= 32, "ot_metrics_update_weighted: 1..32 tasks");
  OT_REQUIRE(nb > 0 && nb <= METRICS_MAX_NB, "ot_metrics_update_weighted: 1..%d thresholds", METRICS_MAX_NB);
  OT_REQUIRE(B > 0, "ot_metrics_update_weighted: empty batch");
  OT_REQUIRE(task_stride >= B, "ot_metrics_update_weighted: task_stride < B");
  OT_REQUIRE(weight_stride == 0 || weight_stride >= B, "ot_metrics_update_weighted: weight_stride is 0 or >= B");
  OT_REQUIRE(ws_bytes >= ot_metrics_weighted_workspace_size(T, B), "ot_metrics_update_weighted: workspace too small");
  OT_REQUIRE((reinterpret_cast<uintptr_t>(probs) & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(weights) & 3) == 0 && (reinterpret_cast<uintptr_t>(bounds) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(counts) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "ot_metrics_update_weighted: misaligned operand");
  const int nblk = metrics_blocks(B);
  const bool vec = ((reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(labels) |
                     reinterpret_cast<uintptr_t>(weights)) & 15) == 0 &&
                   (T == 1 || ((task_stride | weight_stride) & 3) == 0);
  double* part = (double*)workspace;
  unsigned long long* wpart = reinterpret_cast<unsigned long long*>(part + (size_t)T * nblk * 3);
  auto kern = vec ? metrics_update_weighted_kernel<true> : metrics_update_weighted_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(nblk, T), dim3(256), 0, (hipStream_t)stream, probs, labels, weights, B, task_stride,
                     weight_stride, bounds, nb, reinterpret_cast<unsigned long long*>(counts), part, wpart);
  OT_LAUNCH_CHECK("ot_metrics_update_weighted");
  hipLaunchKernelGGL(metrics_fold_weighted_kernel, dim3(T), dim3(64), 0, (hipStream_t)stream, (const double*)part,
                     (const unsigned long long*)wpart, nblk, sums);
  OT_LAUNCH_CHECK("ot_metrics_update_weighted(fold)");
  return OT_OK;
}
