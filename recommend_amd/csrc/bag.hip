// Multi-valued NS features: pooled embedding bags (include/onetrans_hip.h, "embedding bags").
//   ot_ns_bag_pool       out[b][col .. col+E) = sum_j coef[b][j] * table[row_offset + ids[b][j]]  (sum / mean)
//   ot_ns_bag_grad_pack  the (key, gradient row) pairs of every slot, for ot_sparse_adagrad
// A slot whose id is outside [0, num_rows) is empty: never read, coefficient 0, key -1.
//
// Pool: a row gather, bound by HBM / Infinity Cache.  A table row is read as 16-byte pieces: G = E/4 lanes per
// row, padded to the next power of two W (W = G for E = 16, 64, 256; the lanes G..W-1 of a group idle
// otherwise), so a wave holds S = 64/W lane groups.
//   * cap >= S: one (bag, sample) per wave; lane group t takes the slots t, t+S, t+2S, ...
//   * cap <  S: T = the next power of two >= cap lane groups serve one sample, and the wave is shared among
//     S/T consecutive samples of the same bag (E = 16, cap = 4: 4 samples per wave, no idle lane; the lanes of
//     the groups cap..T-1 idle when cap is no power of two).  Waves are never shared between bags: the
//     descriptor stays wave-uniform (scalar registers).
// Summation order (fixed, so the result is bitwise reproducible): each lane group adds its slots in slot order
// (four row loads in flight, added in order), then the T groups of a sample are combined by a butterfly of
// __shfl_xor over the lane distances T/2*W, ..., W: f32 addition is commutative, so both partners of an
// exchange compute the same bits and every group ends with the same sum.  No atomics, no LDS.
// The coefficients w_j * s_b (s_b = 1, or 1.0f / count for 'mean') are stored per slot; the backward multiplies
// the incoming gradient by the stored value, so both passes use the same bits.
#include <algorithm>

#include "common.h"

namespace ot {

constexpr int BAG_MAX = OT_NS_BAG_MAX;

struct BagArgs {                 // the descriptors, by value (validated on the host)
  ot_ns_bag bag[BAG_MAX];
  int64_t base[BAG_MAX + 1];     // first slot position of each bag: base[f+1] = base[f] + B * cap_f
};

__device__ __forceinline__ int bag_pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

__global__ __launch_bounds__(256) void ns_bag_pool_kernel(BagArgs a, int B, float* __restrict__ out, int64_t ld,
                                                          float* __restrict__ coef_out) {
  const ot_ns_bag& d = a.bag[blockIdx.y];
  const int E = d.width, cap = d.cap;
  const int G = E >> 2;
  const int W = bag_pow2_ceil(G);             // lanes of a lane group
  const int S = 64 / W;                       // lane groups of a wave
  const int T = min(S, bag_pow2_ceil(cap));   // lane groups of one sample
  const int spw = S / T;                      // samples of a wave
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int grp = lane / W, lig = lane % W;
  const int t = grp % T;                      // this group's place among its sample's groups
  const int64_t b = wave * spw + grp / T;
  const bool live = b < B;                    // (whole waves past the bag's samples included)
  const int64_t* ids = d.ids + (live ? b : 0) * d.ids_stride;
  const float* wts = d.weights ? d.weights + (live ? b : 0) * d.weights_stride : nullptr;
  // ---- the sample's valid slots (for 'mean'): own slots, then the butterfly
  int cnt = 0;
  if (live)
    for (int j = t; j < cap; j += T) {
      const int64_t id = ids[j];
      cnt += (id >= 0 && id < d.num_rows) ? 1 : 0;
    }
  for (int o = T >> 1; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o * W, 64);
  const float s = d.pooling == OT_BAG_MEAN ? (cnt > 0 ? 1.0f / (float)cnt : 0.f) : 1.f;
  // ---- own slots in slot order, four rows in flight
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float* coef = coef_out + a.base[blockIdx.y] + (live ? b : 0) * cap;
  if (live)
    for (int j0 = t; j0 < cap; j0 += 4 * T) {
      f32x4 v[4];
      float c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = j0 + k * T;
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        c[k] = 0.f;
        if (j < cap) {
          const int64_t id = ids[j];
          const bool ok = id >= 0 && id < d.num_rows;
          c[k] = ok ? (wts ? wts[j] : 1.f) * s : 0.f;
          if (lig == 0) coef[j] = c[k];
          if (ok && lig < G) v[k] = *reinterpret_cast<const f32x4*>(d.table + (d.row_offset + id) * E + 4 * lig);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += v[k] * c[k];
    }
  for (int o = T >> 1; o > 0; o >>= 1) {
    acc.x += __shfl_xor(acc.x, o * W, 64);
    acc.y += __shfl_xor(acc.y, o * W, 64);
    acc.z += __shfl_xor(acc.z, o * W, 64);
    acc.w += __shfl_xor(acc.w, o * W, 64);
  }
  if (live && t == 0 && lig < G) {
    float* dst = out + b * ld + d.col + 4 * lig;
    if ((((uintptr_t)out >> 2) | (uint64_t)ld | (uint64_t)d.col) & 3) {   // a block that starts off a 16-byte line
      dst[0] = acc.x; dst[1] = acc.y; dst[2] = acc.z; dst[3] = acc.w;
    } else {
      *reinterpret_cast<f32x4*>(dst) = acc;
    }
  }
}

// one lane per 16-byte piece of a gradient row: slot p of the call's bags (bag-major, then sample, then slot)
__global__ __launch_bounds__(256) void ns_bag_grad_pack_kernel(BagArgs a, int nbags, int B, int E,
                                                               const float* __restrict__ dmat, int64_t ld,
                                                               const float* __restrict__ coef,
                                                               int64_t* __restrict__ keys, float* __restrict__ grads) {
  const int G = E >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = i / G;
  const int lig = (int)(i % G);
  if (p >= a.base[nbags]) return;
  int f = 0;
  for (int k = 1; k < nbags; ++k)
    if (a.base[k] <= p) f = k;
  const ot_ns_bag& d = a.bag[f];
  const int64_t q = p - a.base[f];
  const int64_t b = q / d.cap;
  const int j = (int)(q % d.cap);
  const int64_t id = d.ids[b * d.ids_stride + j];
  const bool ok = id >= 0 && id < d.num_rows;
  if (lig == 0) keys[p] = ok ? d.row_offset + id : -1;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const float c = coef[p];
    const float* src = dmat + b * ld + d.col + 4 * lig;
    if ((((uintptr_t)dmat >> 2) | (uint64_t)ld | (uint64_t)d.col) & 3)
      g = f32x4{src[0], src[1], src[2], src[3]};
    else
      g = *reinterpret_cast<const f32x4*>(src);
    g = g * c;
  }
  *reinterpret_cast<f32x4*>(grads + p * E + 4 * lig) = g;
}

// shared validation; fills the by-value argument block (ld: the row stride of the matrix the columns index)
static int bag_args(const char* who, const ot_ns_bag* bags, int nbags, int B, int64_t ld, bool pack, BagArgs& a) {
  OT_REQUIRE(bags, "%s: null operand", who);
  OT_REQUIRE(nbags >= 1 && nbags <= BAG_MAX, "%s: nbags=%d must be in [1, %d]", who, nbags, BAG_MAX);
  OT_REQUIRE(B >= 0, "%s: B=%d is negative", who, B);
  a.base[0] = 0;
  for (int f = 0; f < nbags; ++f) {
    const ot_ns_bag& d = bags[f];
    OT_REQUIRE(d.ids && (pack || d.table), "%s: bag %d: null operand", who, f);
    OT_REQUIRE(d.width > 0 && d.width % 4 == 0 && d.width <= OT_NS_BAG_MAX_WIDTH,
               "%s: bag %d: E=%d must be a multiple of 4 <= %d", who, f, d.width, OT_NS_BAG_MAX_WIDTH);
    OT_REQUIRE(!pack || d.width == bags[0].width, "%s: bag %d: E=%d differs from bag 0's %d", who, f, d.width,
               bags[0].width);
    OT_REQUIRE(d.cap >= 1 && d.ids_stride >= d.cap, "%s: bag %d: bad cap / ids_stride", who, f);
    OT_REQUIRE(!d.weights || d.weights_stride >= d.cap, "%s: bag %d: bad weights_stride", who, f);
    OT_REQUIRE(d.pooling == OT_BAG_SUM || d.pooling == OT_BAG_MEAN, "%s: bag %d: unknown pooling %d", who, f,
               d.pooling);
    OT_REQUIRE(!d.weights || d.pooling == OT_BAG_SUM, "%s: bag %d: weights need pooling 'sum'", who, f);
    OT_REQUIRE(d.num_rows > 0 && d.row_offset >= 0, "%s: bag %d: bad row range", who, f);
    OT_REQUIRE(d.col >= 0 && (int64_t)d.col + d.width <= ld, "%s: bag %d: columns [%d, %d) outside ld=%lld", who, f,
               d.col, d.col + d.width, (long long)ld);
    OT_REQUIRE(pack || ((uintptr_t)d.table & 15) == 0, "%s: bag %d: table is not 16-byte aligned", who, f);
    a.bag[f] = d;
    a.base[f + 1] = a.base[f] + (int64_t)B * d.cap;
    OT_REQUIRE(a.base[f + 1] < 2147483647LL, "%s: B * cap out of range", who);
  }
  return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" int ot_ns_bag_pool(const ot_ns_bag* bags, int nbags, int B, float* out, int64_t ld_out, float* coef_out,
                              void* stream) {
  OT_REQUIRE(bags && out && coef_out, "ot_ns_bag_pool: null operand");
  BagArgs a;
  OT_TRY(bag_args("ot_ns_bag_pool", bags, nbags, B, ld_out, false, a));
  if (B == 0) return OT_OK;
  int64_t waves = 1;
  for (int f = 0; f < nbags; ++f) {
    int W = 1, T = 1;
    while (W < bags[f].width / 4) W <<= 1;
    while (T < bags[f].cap && T < 64 / W) T <<= 1;
    const int spw = (64 / W) / T;
    waves = std::max<int64_t>(waves, ((int64_t)B + spw - 1) / spw);
  }
  hipLaunchKernelGGL(ns_bag_pool_kernel, dim3(ceil_div(waves, 4), nbags), dim3(256), 0, (hipStream_t)stream, a, B,
                     out, ld_out, coef_out);
  OT_LAUNCH_CHECK("ot_ns_bag_pool");
  return OT_OK;
}

extern "C" int ot_ns_bag_grad_pack(const ot_ns_bag* bags, int nbags, int B, const float* dmat, int64_t ld,
                                   const float* coef, int64_t* keys, float* grads, void* stream) {
  OT_REQUIRE(bags && dmat && coef && keys && grads, "ot_ns_bag_grad_pack: null operand");
  BagArgs a;
  OT_TRY(bag_args("ot_ns_bag_grad_pack", bags, nbags, B, ld, true, a));
  OT_REQUIRE(((uintptr_t)grads & 15) == 0, "ot_ns_bag_grad_pack: grads is not 16-byte aligned");
  if (B == 0) return OT_OK;
  const int E = bags[0].width;
  const int64_t n = a.base[nbags] * (E / 4);
  hipLaunchKernelGGL(ns_bag_grad_pack_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, nbags, B,
                     E, dmat, ld, coef, keys, grads);
  OT_LAUNCH_CHECK("ot_ns_bag_grad_pack");
  return OT_OK;
}
