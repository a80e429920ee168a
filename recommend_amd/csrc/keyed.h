// Toolkit of the keyed kernels (embedding.hip, shard.hip, metrics_grouped.hip, rank.hip): sort by a key, mark the
// runs of equal keys, carve the workspace.  Header-only: every user instantiates what it calls.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

namespace ot {

// ---- workspace ------------------------------------------------------------------------------------------------
// Hands out consecutive 256-byte-aligned pieces of one workspace.  A null base only measures: every take() gives
// null and total() is the size to ask the caller for.
class Carver {
 public:
  explicit Carver(void* base) : base_((char*)base) {}
  template <class T>
  T* take(size_t count) {
    char* r = base_ ? base_ + off_ : nullptr;
    off_ += (count * sizeof(T) + 255) & ~(size_t)255;
    if (off_ > high_) high_ = off_;
    return (T*)r;
  }
  // overlay: rewind(an earlier offset()) lays the next pieces over the ones taken since
  size_t offset() const { return off_; }
  void rewind(size_t off) { off_ = off; }
  size_t total() const { return high_; }   // the high-water mark across rewinds

 private:
  char* base_;
  size_t off_ = 0, high_ = 0;
};

// ---- rocPRIM ----------------------------------------------------------------------------------------------------
// Each primitive returns an OT_* status, the error described under the caller's label.  tmp, bytes: its temporary
// storage, as in rocPRIM; with a null tmp the call only writes the size it needs to bytes, which is what the
// matching *_bytes query does: a query and its run are the same call.  All are templates, so that a file gets the
// kernels of the primitives it calls and no others.

// stable sort of (key, value) pairs over the key bits [0, end_bit)
template <class Key>
inline int sort_pairs(void* tmp, size_t& bytes, Key* kin, Key* kout, int32_t* vin, int32_t* vout, int64_t n,
                      int end_bit, hipStream_t s, const char* label) {
  return hip_status(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0, end_bit, s), label);
}
template <class Key>
inline size_t sort_pairs_bytes(int64_t n, int end_bit) {
  size_t b = 0;
  (void)sort_pairs<Key>(nullptr, b, nullptr, nullptr, nullptr, nullptr, n, end_bit, 0, "");
  return b;
}

// the same with the values 0, 1, 2, ... (vout: the sorting permutation)
template <class Key>
inline int sort_iota(void* tmp, size_t& bytes, const Key* kin, Key* kout, int32_t* vout, int64_t n, int end_bit,
                     hipStream_t s, const char* label) {
  return hip_status(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, rocprim::counting_iterator<int32_t>(0), vout,
                                              (size_t)n, 0, (unsigned)end_bit, s), label);
}
template <class Key>
inline size_t sort_iota_bytes(int64_t n, int end_bit) {
  size_t b = 0;
  (void)sort_iota<Key>(nullptr, b, nullptr, nullptr, nullptr, n, end_bit, 0, "");
  return b;
}

// keys only, ping-ponging between the two buffers of db (db.current() holds the result)
template <class Key>
inline int sort_keys(void* tmp, size_t& bytes, rocprim::double_buffer<Key>& db, int64_t n, int end_bit,
                     hipStream_t s, const char* label) {
  return hip_status(rocprim::radix_sort_keys(tmp, bytes, db, (size_t)n, 0, (unsigned)end_bit, s), label);
}
template <class Key>
inline size_t sort_keys_bytes(int64_t n, int end_bit) {
  size_t b = 0;
  rocprim::double_buffer<Key> db((Key*)nullptr, (Key*)nullptr);
  (void)sort_keys(nullptr, b, db, n, end_bit, 0, "");
  return b;
}

template <class T>
inline int inclusive_scan(void* tmp, size_t& bytes, T* in, T* out, int64_t n, hipStream_t s, const char* label) {
  return hip_status(rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<T>(), s), label);
}
template <class T>
inline size_t inclusive_scan_bytes(int64_t n) {
  size_t b = 0;
  (void)inclusive_scan<T>(nullptr, b, nullptr, nullptr, n, 0, "");
  return b;
}

template <class T>
inline int exclusive_scan(void* tmp, size_t& bytes, T* in, T* out, int64_t n, hipStream_t s, const char* label) {
  return hip_status(rocprim::exclusive_scan(tmp, bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), s), label);
}
template <class T>
inline size_t exclusive_scan_bytes(int64_t n) {
  size_t b = 0;
  (void)exclusive_scan<T>(nullptr, b, nullptr, nullptr, n, 0, "");
  return b;
}

// ---- runs of equal keys -----------------------------------------------------------------------------------------
// flags[i] = 1 where sorted key i starts a run of equal keys
template <class Key>
__global__ void head_flags_kernel(const Key* __restrict__ sorted, int64_t n, int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

// flags as above, and run[i] = their inclusive scan: the 1-based index of element i's run
template <class Key>
inline int run_index(const Key* sorted, int64_t n, int32_t* flags, int32_t* run, void* tmp, size_t& bytes,
                     hipStream_t s, const char* flags_label, const char* scan_label) {
  hipLaunchKernelGGL(head_flags_kernel<Key>, dim3(ceil_div(n, 256)), dim3(256), 0, s, sorted, n, flags);
  OT_LAUNCH_CHECK(flags_label);
  return inclusive_scan(tmp, bytes, flags, run, n, s, scan_label);
}

// ---- device helpers ---------------------------------------------------------------------------------------------
// largest s in [0, count) with start[s] <= v (start ascending, start[0] <= v)
template <class Index>
__device__ __forceinline__ Index last_start_le(const int32_t* __restrict__ start, Index count, int64_t v) {
  Index lo = 0, hi = count - 1;
  while (lo < hi) {
    const Index mid = (lo + hi + 1) >> 1;
    if (start[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// first index in [0, count) whose owner field (key >> shift) is >= o, in keys sorted by it; count when there is none
template <class Key>
__device__ __forceinline__ int64_t first_owner_ge(const Key* __restrict__ sorted, int64_t count, Key o, int shift) {
  int64_t lo = 0, hi = count;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((sorted[mid] >> shift) < o) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// f32 -> u32 with the same order: -0 -> +0, then the sign flip; every NaN -> the maximum (above +inf: NanHigh) or 0
// (below -inf)
template <bool NanHigh>
__device__ __forceinline__ uint32_t orderable_f32(float s) {
  if (s != s) return NanHigh ? 0xFFFFFFFFu : 0u;
  const uint32_t u = s == 0.f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Inclusive scan over a 256-thread block: returns v summed over the threads 0..threadIdx.x and leaves the four
// waves' totals in wtot (LDS).  One barrier inside; the caller puts another before it calls again.
__device__ __forceinline__ int32_t block_scan_256(int32_t v, int32_t (&wtot)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wtot[w] = x;
  __syncthreads();
  for (int j = 0; j < w; ++j) x += wtot[j];
  return x;
}

}  // namespace ot
