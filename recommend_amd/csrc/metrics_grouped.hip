// Impression-weighted user-level AUC (include/onetrans_hip.h, "grouped AUC"): the paper's second offline metric
// (complete_translation.md:178-180) over a window of (group, label, score) records, one stream-ordered call.
//
// Definition, for one binary task over records (g_i, y_i, s_i), i < n:
//   class        y_i > 0.5, as in ot_metrics_update
//   score order  the order of the f32 values; -0.0 ties with +0.0; every NaN ties with every other NaN and ranks
//                above +inf
//   per group u  n_pos, n_neg and 2U = sum over (pos p, neg q) in u of (2 [s_p > s_q] + [s_p == s_q]), an exact
//                integer; equivalently 2U = sum over pos of (a + b + 1 - 2 start_u) - n_pos (n_pos + 1) with [a, b)
//                the element's tie run in the (group, score)-sorted order and start_u the group's first position
//   valid        n_pos > 0 and n_neg > 0; then AUC_u = (double)2U / (2.0 n_pos n_neg)
//   UAUC         sum_valid n_u AUC_u / sum_valid n_u with n_u = n_pos + n_neg (0 with no valid group: the caller's
//                div_no_nan); also the plain mean over valid groups, their number and their impressions
//
// Pipeline:
//   1. groups, once for all tasks: radix sort of (id, record) over the low group_bits bits, head flags, a scan:
//      the dense index of every record, the distinct ids (ascending, unsigned) and the segment starts
//   2. per task: one 64-bit key per record, dense index << 33 | orderable(score) << 1 | class, radix-sorted (keys
//      only: the statistic needs nothing else of a record).  A group occupies the same positions as in step 1.
//   3. per task: every positive record finds its tie run [a, b) by a galloping search from its own position (a run
//      of one, the usual case, costs the two neighbours) and adds a + b + 1 - 2 start; the sums and the counts are
//      reduced over each wave's stretch of one group (a segmented shuffle scan: a wave's records are sorted by
//      group), then one 64-bit integer atomic per wave and group.  Integer adds commute: the per-group numbers are
//      exact and the same from run to run, and a group of any size costs n_u / 64 atomics, not one thread.
//   4. per task: AUC_u in double per valid group and the four sums, reduced thread -> wave -> workgroup ->
//      workgroups in index order through the workspace (no float atomics).  Which thread takes which group depends
//      on the group's dense index and n only, so agg is also the same under any permutation of the records.
#include "keyed.h"

namespace ot {

constexpr int GAUC_MAX_BLOCKS = 256;  // workgroups of the finalise pass per task (the rest is grid-strided)

inline int gauc_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > GAUC_MAX_BLOCKS ? GAUC_MAX_BLOCKS : b));
}

// flags, pos: run_index of the sorted ids (1 <= pos[i] <= n).  dense[record] = its group's index; seg_start[0..G] the
// groups' first sorted positions (seg_start[G] = n); ids[g] the distinct ids.
__global__ void gauc_segments_kernel(const uint64_t* __restrict__ k, const int32_t* __restrict__ rec,
                                     const int32_t* __restrict__ flags, const int32_t* __restrict__ pos, int64_t n,
                                     int32_t* dense, int32_t* seg_start, int32_t* nuniq, int64_t* num_groups,
                                     int64_t* ids) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = pos[i] - 1;
  dense[rec[i]] = g;
  if (flags[i]) {
    seg_start[g] = (int32_t)i;
    if (ids) ids[g] = (int64_t)k[i];
  }
  if (i == n - 1) {
    seg_start[g + 1] = (int32_t)n;
    nuniq[0] = g + 1;
    num_groups[0] = g + 1;
  }
}

__global__ void gauc_pack_kernel(const int32_t* __restrict__ dense, const float* __restrict__ scores,
                                 const float* __restrict__ labels, int64_t n, uint64_t* keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = ((uint64_t)(uint32_t)dense[i] << 33) | ((uint64_t)orderable_f32<true>(scores[i]) << 1) |
            (labels[i] > 0.5f ? 1u : 0u);
}

// One sorted record per thread.  stat[g] = {n_pos, sum over the group's positives of (a + b + 1 - 2 start)}, zeroed
// by the caller.
__global__ __launch_bounds__(256) void gauc_stat_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                        const int32_t* __restrict__ seg_start,
                                                        unsigned long long* stat) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t d = 0xFFFFFFFFu;   // past the end: no group (a dense index is below 2^31)
  unsigned long long cnt = 0, sum = 0;
  if (i < n) {
    const uint64_t k = keys[i], r = k >> 1;
    d = (uint32_t)(r >> 32);
    if (k & 1) {
      // a: the first position of the tie run (keys[lo] >> 1 == r throughout)
      int64_t lo = i, step = 1;
      while (lo >= step && (keys[lo - step] >> 1) == r) {
        lo -= step;
        step <<= 1;
      }
      int64_t left = lo >= step ? lo - step : -1, right = lo;   // left: differs (or -1); right: equal
      while (right - left > 1) {
        const int64_t mid = (left + right) >> 1;
        if ((keys[mid] >> 1) == r) right = mid;
        else left = mid;
      }
      const int64_t a = right;
      // b: one past its last position
      int64_t hi = i;
      step = 1;
      while (hi + step < n && (keys[hi + step] >> 1) == r) {
        hi += step;
        step <<= 1;
      }
      left = hi;                                 // equal
      right = hi + step < n ? hi + step : n;     // differs (or n)
      while (right - left > 1) {
        const int64_t mid = (left + right) >> 1;
        if ((keys[mid] >> 1) == r) left = mid;
        else right = mid;
      }
      cnt = 1;
      sum = (unsigned long long)(a + right + 1 - 2 * (int64_t)seg_start[d]);
    }
  }
  // inclusive scan over the wave's stretch of each group (the groups are sorted, so equal d at distance o means
  // equal d in between); the stretch's last lane then holds its totals
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t d2 = __shfl_up(d, o, 64);
    const unsigned long long c2 = __shfl_up(cnt, o, 64), s2 = __shfl_up(sum, o, 64);
    if (lane >= o && d2 == d) {
      cnt += c2;
      sum += s2;
    }
  }
  const uint32_t dn = __shfl_down(d, 1, 64);
  if (d != 0xFFFFFFFFu && (lane == 63 || dn != d) && cnt) {
    atomicAdd(&stat[2 * (int64_t)d], cnt);
    atomicAdd(&stat[2 * (int64_t)d + 1], sum);
  }
}

// grid gauc_blocks(n), 256 threads: thread i of workgroup b takes the groups b*256 + i, + gridDim.x*256, ...
// part[b*4 + {0,1,2,3}] = this workgroup's {sum n_u AUC_u, sum AUC_u, sum n_u, #valid}; gstats (or null): the
// task's [n][3] rows {n_pos, n_neg, 2U} of the distinct groups.
__global__ __launch_bounds__(256) void gauc_finalise_kernel(const unsigned long long* __restrict__ stat,
                                                            const int32_t* __restrict__ seg_start,
                                                            const int32_t* __restrict__ nuniq, int64_t* gstats,
                                                            double* part) {
  __shared__ double red[4][4];
  const int G = nuniq[0], tid = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t g = (int64_t)blockIdx.x * 256 + tid; g < G; g += (int64_t)gridDim.x * 256) {
    const int64_t nu = seg_start[g + 1] - seg_start[g];
    const int64_t npos = (int64_t)stat[2 * g], nneg = nu - npos;
    const int64_t u2 = (int64_t)stat[2 * g + 1] - npos * (npos + 1);
    if (gstats) {
      gstats[3 * g] = npos;
      gstats[3 * g + 1] = nneg;
      gstats[3 * g + 2] = u2;
    }
    if (npos > 0 && nneg > 0) {
      const double auc = (double)u2 / (2.0 * (double)npos * (double)nneg);
      acc[0] += (double)nu * auc;
      acc[1] += auc;
      acc[2] += (double)nu;
      acc[3] += 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k] = wave_sum(acc[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < 4) part[(int64_t)blockIdx.x * 4 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// grid T, 256 threads: agg[t] = the workgroups' partials folded in index order (a masked task: zeros).  The
// partials are fetched by all threads at once and summed from LDS (one thread's chain of dependent global loads
// took as long as a sort pass).
__global__ __launch_bounds__(256) void gauc_fold_kernel(const double* __restrict__ part, int nblk,
                                                        uint32_t task_mask, double* agg) {
  __shared__ double sp[GAUC_MAX_BLOCKS * 4];
  const int t = blockIdx.x, k = threadIdx.x;
  const bool on = (task_mask >> t) & 1u;
  if (on)
    for (int i = k; i < nblk * 4; i += 256) sp[i] = part[(int64_t)t * nblk * 4 + i];
  __syncthreads();
  if (k >= 4) return;
  double s = 0.0;
  if (on)
    for (int b = 0; b < nblk; ++b) s += sp[b * 4 + k];
  agg[t * 4 + k] = s;
}

struct GaucWs {
  // persistent over the call
  int32_t *dense, *seg_start, *nuniq;
  double* part;
  void* tmp;
  size_t tmp_bytes;
  // step 1 (dead once the segments are known) ...
  uint64_t* k_out;
  int32_t *v_out, *flags, *pos;
  // ... and steps 2-4, in the same bytes
  uint64_t *key_a, *key_b;
  unsigned long long* stat;
  size_t total;
};

inline int gauc_key_bits(int64_t n) {   // dense indices are below n
  int b = 0;
  while (b < 31 && ((int64_t)1 << b) < n) ++b;
  return 33 + b;
}

GaucWs gauc_carve(void* base, int T, int64_t n, int group_bits) {
  GaucWs w{};
  w.tmp_bytes = std::max({sort_iota_bytes<uint64_t>(n, group_bits), sort_keys_bytes<uint64_t>(n, gauc_key_bits(n)),
                          inclusive_scan_bytes<int32_t>(n)});
  Carver c(base);
  w.dense = c.take<int32_t>(n);
  w.seg_start = c.take<int32_t>(n + 1);
  w.nuniq = c.take<int32_t>(1);
  w.part = c.take<double>((size_t)T * gauc_blocks(n) * 4);
  w.tmp = c.take<char>(w.tmp_bytes);
  const size_t shared = c.offset();
  w.k_out = c.take<uint64_t>(n);
  w.v_out = c.take<int32_t>(n);
  w.flags = c.take<int32_t>(n);
  w.pos = c.take<int32_t>(n);
  c.rewind(shared);
  w.key_a = c.take<uint64_t>(n);
  w.key_b = c.take<uint64_t>(n);
  w.stat = c.take<unsigned long long>(2 * (size_t)n);
  w.total = c.total();
  return w;
}

}  // namespace ot

using namespace ot;

extern "C" size_t ot_grouped_auc_workspace_size(int T, int64_t n, int group_bits) {
  if (T < 1 || T > 32 || n < 1 || n >= 2147483648LL || group_bits < 1 || group_bits > 64) return 0;
  return gauc_carve(nullptr, T, n, group_bits).total;
}

extern "C" int ot_grouped_auc(const int64_t* groups, const float* scores, const float* labels, int T, int64_t n,
                              int64_t task_stride, int group_bits, uint32_t task_mask, double* agg,
                              int64_t* num_groups, int64_t* group_ids, int64_t* group_stats, void* workspace,
                              size_t ws_bytes, void* stream) {
  OT_REQUIRE(groups && scores && labels && agg && num_groups && workspace, "ot_grouped_auc: null operand");
  OT_REQUIRE(T > 0 && T <= 32, "ot_grouped_auc: 1..32 tasks");
  OT_REQUIRE(n > 0 && n < 2147483648LL, "ot_grouped_auc: n out of range (1 <= n < 2^31)");
  OT_REQUIRE(task_stride >= n, "ot_grouped_auc: task_stride < n");
  OT_REQUIRE(group_bits >= 1 && group_bits <= 64, "ot_grouped_auc: group_bits out of range (1..64)");
  OT_REQUIRE((reinterpret_cast<uintptr_t>(scores) & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(groups) & 7) == 0 && (reinterpret_cast<uintptr_t>(agg) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(num_groups) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(group_ids) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(group_stats) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
             "ot_grouped_auc: misaligned operand");
  GaucWs w = gauc_carve(workspace, T, n, group_bits);
  OT_REQUIRE(ws_bytes >= w.total, "ot_grouped_auc: workspace too small (%zu < %zu)", ws_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  const unsigned g1 = ceil_div(n, 256);
  const int nblk = gauc_blocks(n);

  // 1. the groups
  OT_TRY(sort_iota(w.tmp, w.tmp_bytes, reinterpret_cast<const uint64_t*>(groups), w.k_out, w.v_out, n, group_bits, s,
                   "ot_grouped_auc(group sort)"));
  OT_TRY(run_index(w.k_out, n, w.flags, w.pos, w.tmp, w.tmp_bytes, s, "ot_grouped_auc(flags)",
                   "ot_grouped_auc(scan)"));
  hipLaunchKernelGGL(gauc_segments_kernel, dim3(g1), dim3(256), 0, s, w.k_out, w.v_out, w.flags, w.pos, n, w.dense,
                     w.seg_start, w.nuniq, num_groups, group_ids);
  OT_LAUNCH_CHECK("ot_grouped_auc(segments)");
  if (group_stats)
    OT_TRY(hip_status(hipMemsetAsync(group_stats, 0, (size_t)T * n * 3 * sizeof(int64_t), s), "ot_grouped_auc(clear)"));

  // 2-4. per binary task
  for (int t = 0; t < T; ++t) {
    if (!((task_mask >> t) & 1u)) continue;
    hipLaunchKernelGGL(gauc_pack_kernel, dim3(g1), dim3(256), 0, s, w.dense, scores + (int64_t)t * task_stride,
                       labels + (int64_t)t * task_stride, n, w.key_a);
    OT_LAUNCH_CHECK("ot_grouped_auc(pack)");
    rocprim::double_buffer<uint64_t> db(w.key_a, w.key_b);
    OT_TRY(sort_keys(w.tmp, w.tmp_bytes, db, n, gauc_key_bits(n), s, "ot_grouped_auc(score sort)"));
    OT_TRY(hip_status(hipMemsetAsync(w.stat, 0, (size_t)n * 16, s), "ot_grouped_auc(clear)"));
    hipLaunchKernelGGL(gauc_stat_kernel, dim3(g1), dim3(256), 0, s, db.current(), n, w.seg_start, w.stat);
    OT_LAUNCH_CHECK("ot_grouped_auc(stat)");
    hipLaunchKernelGGL(gauc_finalise_kernel, dim3(nblk), dim3(256), 0, s, w.stat, w.seg_start, w.nuniq,
                       group_stats ? group_stats + (int64_t)t * n * 3 : nullptr, w.part + (int64_t)t * nblk * 4);
    OT_LAUNCH_CHECK("ot_grouped_auc(finalise)");
  }
  hipLaunchKernelGGL(gauc_fold_kernel, dim3(T), dim3(256), 0, s, w.part, nblk, task_mask, agg);
  OT_LAUNCH_CHECK("ot_grouped_auc(fold)");
  return OT_OK;
}
