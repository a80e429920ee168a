// Per-request top-K ranking of scored candidates (include/onetrans_hip.h, "ranking"): the serving step after
// stage II.  C candidates carry T task probabilities (task-major, what the head writes) and a request index; the
// answer is, per request, the K best candidates under one fused score, in rank order, in one stream-ordered call.
//
// Definition (the header has the full text):
//   fused score  f32, in task order: sum  f = fmaf(w_t, p_t, f) from 0;  product  f = f * p_t over w_t != 0 from 1
//   key          orderable(f) << 32 | (0xFFFFFFFF - c): NaN below -inf, -0 ties with +0, equal scores to the lower
//                candidate index.  Keys are distinct, so every answer is unique: whatever order the atomics below
//                arrive in, the output bits are the same.
//   membership   0 <= req[c] < R; any other value excludes the candidate (it is counted and scattered nowhere)
//
// Pipeline (one memset and four launches):
//   1. fuse + count   one thread per candidate: f[c], and its arrival number in its request from an int32 atomic
//                     add on the request's counter, one per run of neighbouring lanes with the same request
//                     (integer adds commute: the totals are exact)
//   2. scan           one workgroup: the exclusive scan of the counters, the requests' segment starts
//   3. scatter        key[c] to start[req[c]] + arrival number (a request's keys in arbitrary order)
//   4. select         one 256-thread workgroup per request: radix select of the k-th largest key, 8 bits a pass
//                     from the top (LDS histogram with integer atomics, the segment streamed from global memory
//                     each pass: any n_r), stopping as soon as the threshold digit's bucket is wanted whole; the
//                     keys >= threshold compacted into LDS (at most 1024), bitonic-sorted descending, written out
//                     with the padding slots and the count.  n_r <= K skips the select (threshold 0).
#include "keyed.h"

namespace ot {

constexpr int RANK_MAX_K = 1024;
constexpr int RANK_MAX_T = 32;

struct RankWeights {
  float w[RANK_MAX_T];
};

__device__ __forceinline__ uint64_t rank_key(float f, uint32_t c) {
  return ((uint64_t)orderable_f32<false>(f) << 32) | (uint64_t)(0xFFFFFFFFu - c);   // NaN -> 0, below -inf
}

// One thread per candidate.  cnt[R] zeroed by the caller; arrival[c] is written for members only.
__global__ __launch_bounds__(256) void rank_fuse_kernel(const float* __restrict__ probs, int64_t task_stride, int T,
                                                        RankWeights wts, int mode, const int32_t* __restrict__ req,
                                                        int64_t C, int R, float* __restrict__ fused,
                                                        int32_t* __restrict__ arrival, int32_t* cnt) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t r = -1;                                         // no request: past the end, or excluded
  if (c < C) {
    float f;
    if (mode == OT_RANK_SUM) {
      f = 0.0f;
      for (int t = 0; t < T; ++t) f = __builtin_fmaf(wts.w[t], probs[(int64_t)t * task_stride + c], f);
    } else {
      f = 1.0f;
      for (int t = 0; t < T; ++t)
        if (wts.w[t] != 0.0f) f = __fmul_rn(f, probs[(int64_t)t * task_stride + c]);
    }
    fused[c] = f;
    const int32_t q = req[c];
    if (q >= 0 && q < R) r = q;
  }
  // One atomic per run of neighbouring lanes with the same request, by the run's first lane (candidates usually
  // arrive grouped by request: one returning atomic per candidate on a request's single counter serialised at
  // its L2 channel, measured 150 us for 64 requests of 512).  Arrival numbers stay a permutation of 0..n_r-1.
  const int32_t prev = __shfl_up(r, 1, 64);
  const uint64_t heads = __ballot(lane == 0 || prev != r);
  const uint64_t upto = (2ull << lane) - 1;               // lanes 0..lane (lane 63: all)
  const int first = 63 - __builtin_clzll(heads & upto);   // this lane's run starts here (bit 0 is always set)
  const uint64_t later = heads & ~upto;
  const int end = later ? __builtin_ctzll(later) : 64;    // and ends before here
  int32_t base = 0;
  if (first == lane && r >= 0) base = atomicAdd(&cnt[r], end - lane);
  base = __shfl(base, first, 64);
  if (r >= 0) arrival[c] = base + (lane - first);
}

// One workgroup: start[0..R] = the exclusive scan of cnt[0..R) (start[R] = the number of members).
__global__ __launch_bounds__(256) void rank_scan_kernel(const int32_t* __restrict__ cnt, int R,
                                                        int32_t* __restrict__ start) {
  __shared__ int32_t wtot[4];
  const int tid = threadIdx.x;
  int32_t carry = 0;
  for (int base = 0; base < R; base += 256) {
    const int r = base + tid;
    const int32_t v = r < R ? cnt[r] : 0;
    const int32_t x = block_scan_256(v, wtot);
    if (r < R) start[r] = carry + x - v;
    carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (tid == 0) start[R] = carry;
}

__global__ __launch_bounds__(256) void rank_scatter_kernel(const float* __restrict__ fused,
                                                           const int32_t* __restrict__ req,
                                                           const int32_t* __restrict__ arrival,
                                                           const int32_t* __restrict__ start, int64_t C, int R,
                                                           uint64_t* __restrict__ keys) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int32_t r = req[c];
  if (r >= 0 && r < R) keys[(int64_t)start[r] + arrival[c]] = rank_key(fused[c], (uint32_t)c);
}

// grid R, 256 threads.  keys: the requests' segments (start[r] .. start[r + 1]); fused: f[C].
__global__ __launch_bounds__(256) void rank_select_kernel(const uint64_t* __restrict__ keys,
                                                          const int32_t* __restrict__ start,
                                                          const float* __restrict__ fused, int K,
                                                          int32_t* __restrict__ top_idx, float* __restrict__ top_score,
                                                          int32_t* __restrict__ count) {
  __shared__ uint64_t list[RANK_MAX_K];
  __shared__ int32_t hist[256];
  __shared__ int32_t wtot[4];
  __shared__ int32_t sel[3];     // the threshold digit, what is still wanted inside its bucket, the bucket's size
  __shared__ int32_t nlist;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int32_t s0 = start[r], n = start[r + 1] - s0;
  const int k = n < K ? n : K;
  const uint64_t* seg = keys + s0;
  int32_t* oi = top_idx + (int64_t)r * K;
  float* os = top_score + (int64_t)r * K;
  if (tid == 0) count[r] = k;
  for (int j = k + tid; j < K; j += 256) {
    oi[j] = -1;
    os[j] = -__builtin_inff();
  }
  if (k == 0) return;                                     // workgroup-uniform

  // the threshold: exactly k keys are >= thr (a real key is never 0: its low word is 0xFFFFFFFF - c >= 2^31)
  uint64_t thr = 0;
  if (n > K) {
    int32_t want = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
      const uint64_t above = shift == 56 ? 0ull : ~0ull << (shift + 8);   // the digits already fixed
      hist[tid] = 0;
      __syncthreads();
      for (int32_t i = tid; i < n; i += 256) {
        const uint64_t key = seg[i];
        if ((key & above) == thr) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
      }
      __syncthreads();
      // inclusive scan from the largest digit down: thread t holds digit 255 - t
      const int32_t v = hist[255 - tid];
      const int32_t x = block_scan_256(v, wtot);
      if (x - v < want && want <= x) {                    // exactly one thread: the k-th key's digit
        sel[0] = 255 - tid;
        sel[1] = want - (x - v);
        sel[2] = v;
      }
      __syncthreads();
      thr |= (uint64_t)sel[0] << shift;
      want = sel[1];
      if (sel[2] == want) break;                          // the whole bucket is wanted: the low bits stay 0
    }
  }

  // compaction (arbitrary order) and the padding up to a power of two
  int P = 1;
  while (P < k) P <<= 1;
  if (tid == 0) nlist = 0;
  for (int j = k + tid; j < P; j += 256) list[j] = 0;
  __syncthreads();
  for (int32_t i = tid; i < n; i += 256) {
    const uint64_t key = seg[i];
    if (key >= thr) {
      const int32_t slot = atomicAdd(&nlist, 1);
      if (slot < k) list[slot] = key;
    }
  }
  // bitonic sort, descending
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (P >> 1); t += 256) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool desc = (i & size) == 0;
        const uint64_t a = list[i], b = list[j];
        if (desc ? a < b : a > b) {
          list[i] = b;
          list[j] = a;
        }
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < k; j += 256) {
    const uint32_t c = 0xFFFFFFFFu - (uint32_t)list[j];
    oi[j] = (int32_t)c;
    os[j] = fused[c];
  }
}

struct RankWs {
  float* fused;
  int32_t *arrival, *cnt, *start;
  uint64_t* keys;
  size_t total;
};

RankWs rank_carve(void* base, int R, int64_t C) {
  RankWs w{};
  Carver c(base);
  w.keys = c.take<uint64_t>(C);
  w.fused = c.take<float>(C);
  w.arrival = c.take<int32_t>(C);
  w.cnt = c.take<int32_t>(R);
  w.start = c.take<int32_t>((size_t)R + 1);
  w.total = c.total();
  return w;
}

}  // namespace ot

using namespace ot;

extern "C" size_t ot_rank_topk_workspace_size(int R, int64_t C, int K) {
  if (R < 0 || C < 0 || C > (int64_t)INT32_MAX || K < 1 || K > RANK_MAX_K) return 0;
  return rank_carve(nullptr, R, C).total;
}

extern "C" int ot_rank_topk(const float* probs, int64_t task_stride, int T, const float* weights_host, int mode,
                            const int32_t* req, int64_t C, int R, int K, int32_t* top_idx, float* top_score,
                            int32_t* count, float* fused_out, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(K >= 1 && K <= RANK_MAX_K, "ot_rank_topk: K=%d out of range (1..%d)", K, RANK_MAX_K);
  OT_REQUIRE(T >= 1 && T <= RANK_MAX_T, "ot_rank_topk: 1..%d tasks (T=%d)", RANK_MAX_T, T);
  OT_REQUIRE(C >= 0 && C <= (int64_t)INT32_MAX, "ot_rank_topk: C out of range (0 <= C <= INT32_MAX)");
  OT_REQUIRE(R >= 0, "ot_rank_topk: R=%d is negative", R);
  OT_REQUIRE(mode == OT_RANK_SUM || mode == OT_RANK_PRODUCT, "ot_rank_topk: unknown mode %d", mode);
  OT_REQUIRE(task_stride >= C, "ot_rank_topk: task_stride < C");
  const size_t need = rank_carve(nullptr, R, C).total;
  OT_REQUIRE(ws_bytes >= need, "ot_rank_topk: workspace too small (%zu < %zu)", ws_bytes, need);
  OT_REQUIRE(weights_host && workspace && (R == 0 || (top_idx && top_score && count)) && (C == 0 || (probs && req)),
             "ot_rank_topk: null operand");
  OT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ot_rank_topk: misaligned workspace");
  const RankWs w = rank_carve(workspace, R, C);
  hipStream_t s = (hipStream_t)stream;
  float* fused = fused_out ? fused_out : w.fused;
  if (R > 0) OT_TRY(hip_status(hipMemsetAsync(w.cnt, 0, (size_t)R * 4, s), "ot_rank_topk(clear)"));
  if (C > 0) {
    RankWeights wts{};
    for (int t = 0; t < T; ++t) wts.w[t] = weights_host[t];
    hipLaunchKernelGGL(rank_fuse_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, probs, task_stride, T, wts, mode,
                       req, C, R, fused, w.arrival, w.cnt);
    OT_LAUNCH_CHECK("ot_rank_topk(fuse)");
  }
  if (R == 0) return OT_OK;
  hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(256), 0, s, w.cnt, R, w.start);
  OT_LAUNCH_CHECK("ot_rank_topk(scan)");
  if (C > 0) {
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, fused, req, w.arrival, w.start,
                       C, R, w.keys);
    OT_LAUNCH_CHECK("ot_rank_topk(scatter)");
  }
  hipLaunchKernelGGL(rank_select_kernel, dim3(R), dim3(256), 0, s, w.keys, w.start, fused, K, top_idx, top_score,
                     count);
  OT_LAUNCH_CHECK("ot_rank_topk(select)");
  return OT_OK;
}
