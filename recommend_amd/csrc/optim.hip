// Dense optimizer step: per-variable tf.clip_by_norm (train.py:134-135) followed by Keras-2.12
// RMSprop with momentum (train.py:64-70, 138; config.py:39-48, momentum 0.99999):
//   v = rho v + (1-rho) g^2 ; inc = lr g rsqrt(v + eps) ; m = mom m + inc ; w -= m
// Variables are 2-D strided segments {offset, rows, cols, row_stride} of ONE flat parameter /
// gradient / state buffer (a Keras variable such as Wq_dedicated[3] is a column slice of the fused
// [G, d, 3d] QKV bank).  Three launches, no host sync, deterministic (fixed-order partial sums).
// ot_clip_adam is the same clip followed by Keras-2.12 Adam (train.py:57-63, 71-74): see adam_update.
#include <cmath>

#include "common.h"

namespace ot {

constexpr int OPT_CHUNK = 4096;   // elements per block

__device__ __forceinline__ int64_t seg_addr(const int64_t* sg, int64_t e) {
  const int64_t cols = sg[2];
  return sg[0] + (e / cols) * sg[3] + (e % cols);
}

__global__ __launch_bounds__(256) void seg_sumsq_kernel(const float* __restrict__ g, const int64_t* __restrict__ segs,
                                                        int nchunk, float* part) {
  const int seg = blockIdx.y, ch = blockIdx.x;
  const int64_t* sg = segs + 4 * seg;
  const int64_t n = sg[1] * sg[2];
  const int64_t e0 = (int64_t)ch * OPT_CHUNK;
  float s = 0.f;
  for (int64_t e = e0 + threadIdx.x; e < n && e < e0 + OPT_CHUNK; e += 256) {
    const float v = g[seg_addr(sg, e)];
    s += v * v;
  }
  s = block_sum_256(s);
  if (threadIdx.x == 0) part[(int64_t)seg * nchunk + ch] = s;
}

__global__ void seg_scale_kernel(const float* __restrict__ part, const int64_t* __restrict__ segs, int nseg, int nchunk,
                                 float clip, float* scale) {
  const int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= nseg) return;
  const int64_t n = segs[4 * seg + 1] * segs[4 * seg + 2];
  const int used = (int)((n + OPT_CHUNK - 1) / OPT_CHUNK);
  float s = 0.f;
  for (int c = 0; c < used; ++c) s += part[(int64_t)seg * nchunk + c];
  const float l2 = sqrtf(s);
  scale[seg] = clip > 0.f ? clip / fmaxf(l2, clip) : 1.f;
}

__global__ __launch_bounds__(256) void rmsprop_kernel(float* w, const float* __restrict__ g, float* v, float* m,
                                                      const int64_t* __restrict__ segs, const float* __restrict__ scale,
                                                      float lr, float rho, float eps, float mom) {
  const int seg = blockIdx.y, ch = blockIdx.x;
  const int64_t* sg = segs + 4 * seg;
  const int64_t n = sg[1] * sg[2];
  const int64_t e0 = (int64_t)ch * OPT_CHUNK;
  const float sc = scale[seg];
  for (int64_t e = e0 + threadIdx.x; e < n && e < e0 + OPT_CHUNK; e += 256) {
    const int64_t a = seg_addr(sg, e);
    const float gg = g[a] * sc;
    const float vv = rho * v[a] + (1.f - rho) * gg * gg;
    const float inc = lr * gg * rsqrtf(vv + eps);
    v[a] = vv;
    if (mom > 0.f) {
      const float mm = mom * m[a] + inc;
      m[a] = mm;
      w[a] -= mm;
    } else {
      w[a] -= inc;
    }
  }
}

// Keras-2.12 Adam.update_step on the clipped gradient (alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) from the host):
//   m += (g - m)(1 - beta1) ; v += (g^2 - v)(1 - beta2) ; w -= (m alpha) / (sqrt(v) + eps)
// eps is added OUTSIDE the square root (RMSprop above has it inside), so this is a true sqrt and a true divide.
__device__ __forceinline__ void adam_update(float& w, float g, float& m, float& v, float alpha, float omb1, float omb2,
                                            float eps) {
  m += (g - m) * omb1;
  v += (g * g - v) * omb2;
  w -= (m * alpha) / (sqrtf(v) + eps);
}

// One thread's walk over a chunk, W elements at a time: (row, column) come from one divide at the thread's first
// element and then advance by the block's stride (256 W elements = dq rows + dr columns), with no divide per element.
// W = 4 needs offset, cols and row_stride (and the four base pointers) to be multiples of 4 floats: a group of four
// consecutive segment elements then lies in one row at a 16-byte aligned address, and n = rows * cols is a multiple
// of 4, so no group straddles the segment's end.
template <int W>
__device__ __forceinline__ void adam_walk(float* w, const float* __restrict__ g, float* m, float* v, int64_t off,
                                          int64_t cols, int64_t stride, int64_t e0, int64_t end, float sc, float alpha,
                                          float omb1, float omb2, float eps) {
  constexpr int STEP = 256 * W;
  const int64_t dq = cols > STEP ? 0 : STEP / (int)cols;
  const int64_t dr = STEP - dq * cols;
  int64_t e = e0 + (int64_t)threadIdx.x * W;
  int64_t r = e / cols, c = e - r * cols;
  for (; e < end; e += STEP) {
    const int64_t a = off + r * stride + c;
    if constexpr (W == 4) {
      f32x4 ww = *reinterpret_cast<const f32x4*>(w + a);
      const f32x4 gg = *reinterpret_cast<const f32x4*>(g + a) * sc;
      f32x4 mm = *reinterpret_cast<const f32x4*>(m + a);
      f32x4 vv = *reinterpret_cast<const f32x4*>(v + a);
#pragma unroll
      for (int k = 0; k < 4; ++k) {   // (a vector's element cannot bind to a reference)
        float w1 = ww[k], m1 = mm[k], v1 = vv[k];
        adam_update(w1, gg[k], m1, v1, alpha, omb1, omb2, eps);
        ww[k] = w1;
        mm[k] = m1;
        vv[k] = v1;
      }
      *reinterpret_cast<f32x4*>(m + a) = mm;
      *reinterpret_cast<f32x4*>(v + a) = vv;
      *reinterpret_cast<f32x4*>(w + a) = ww;
    } else {
      float ww = w[a], mm = m[a], vv = v[a];
      adam_update(ww, g[a] * sc, mm, vv, alpha, omb1, omb2, eps);
      m[a] = mm;
      v[a] = vv;
      w[a] = ww;
    }
    c += dr;
    r += dq;
    if (c >= cols) {
      c -= cols;
      ++r;
    }
  }
}

// Same (chunk, segment) grid as rmsprop_kernel.  ptr_vec: the host found w, g, m, v 16-byte aligned.
__global__ __launch_bounds__(256) void adam_kernel(float* w, const float* __restrict__ g, float* m, float* v,
                                                   const int64_t* __restrict__ segs, const float* __restrict__ scale,
                                                   float alpha, float omb1, float omb2, float eps, int ptr_vec) {
  const int seg = blockIdx.y;
  const int64_t* sg = segs + 4 * seg;
  const int64_t off = sg[0], cols = sg[2], stride = sg[3];
  const int64_t n = sg[1] * cols;
  const int64_t e0 = (int64_t)blockIdx.x * OPT_CHUNK;
  if (e0 >= n) return;
  const int64_t end = n < e0 + OPT_CHUNK ? n : e0 + OPT_CHUNK;
  const float sc = scale[seg];
  if (ptr_vec && ((off | cols | stride) & 3) == 0)
    adam_walk<4>(w, g, m, v, off, cols, stride, e0, end, sc, alpha, omb1, omb2, eps);
  else
    adam_walk<1>(w, g, m, v, off, cols, stride, e0, end, sc, alpha, omb1, omb2, eps);
}

inline int nchunks_for(int64_t max_seg_elems) { return (int)((max_seg_elems + OPT_CHUNK - 1) / OPT_CHUNK); }

}  // namespace ot

using namespace ot;

extern "C" size_t ot_clip_rmsprop_workspace_size(int nseg, int64_t max_seg_elems) {
  return ((size_t)nseg * nchunks_for(max_seg_elems) + nseg) * sizeof(float);
}

extern "C" int ot_clip_rmsprop(float* w, float* g, float* v, float* m, const int64_t* segs_dev, int nseg,
                               int64_t max_seg_elems, float lr, float rho, float eps, float momentum, float clip,
                               void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(w && g && v && m && segs_dev && workspace, "ot_clip_rmsprop: null operand");
  OT_REQUIRE(ws_bytes >= ot_clip_rmsprop_workspace_size(nseg, max_seg_elems), "ot_clip_rmsprop: workspace too small");
  if (nseg == 0) return OT_OK;
  const int nch = nchunks_for(max_seg_elems);
  float* part = (float*)workspace;
  float* scale = part + (size_t)nseg * nch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(seg_sumsq_kernel, dim3(nch, nseg), dim3(256), 0, s, g, segs_dev, nch, part);
  OT_LAUNCH_CHECK("ot_clip_rmsprop(sumsq)");
  hipLaunchKernelGGL(seg_scale_kernel, dim3(ceil_div(nseg, 256)), dim3(256), 0, s, part, segs_dev, nseg, nch, clip,
                     scale);
  OT_LAUNCH_CHECK("ot_clip_rmsprop(scale)");
  hipLaunchKernelGGL(rmsprop_kernel, dim3(nch, nseg), dim3(256), 0, s, w, g, v, m, segs_dev, scale, lr, rho, eps,
                     momentum);
  OT_LAUNCH_CHECK("ot_clip_rmsprop(apply)");
  return OT_OK;
}

extern "C" size_t ot_clip_adam_workspace_size(int nseg, int64_t max_seg_elems) {
  return ((size_t)nseg * nchunks_for(max_seg_elems) + nseg) * sizeof(float);
}

extern "C" int ot_clip_adam(float* w, float* g, float* m, float* v, const int64_t* segs_dev, int nseg,
                            int64_t max_seg_elems, float lr, float beta1, float beta2, float eps, int64_t step,
                            float clip, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(w && g && m && v && segs_dev && workspace, "ot_clip_adam: null operand");
  OT_REQUIRE(nseg >= 0 && max_seg_elems >= 0, "ot_clip_adam: bad sizes");
  OT_REQUIRE(ws_bytes >= ot_clip_adam_workspace_size(nseg, max_seg_elems), "ot_clip_adam: workspace too small");
  OT_REQUIRE(step >= 1, "ot_clip_adam: step is the 1-based index of the step being applied (got %lld)",
             (long long)step);
  OT_REQUIRE(beta1 >= 0.f && beta1 < 1.f, "ot_clip_adam: beta1 must be in [0, 1)");
  OT_REQUIRE(beta2 >= 0.f && beta2 <= 1.f, "ot_clip_adam: beta2 must be in [0, 1]");
  if (nseg == 0) return OT_OK;
  // beta2 == 1 (the reference's default optimizer_config carries it): alpha = 0 and 1 - beta2 = 0, so w and v stay
  const double alpha =
      (double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)step)) / (1.0 - std::pow((double)beta1, (double)step));
  const int ptr_vec = (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const int nch = nchunks_for(max_seg_elems);
  float* part = (float*)workspace;
  float* scale = part + (size_t)nseg * nch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(seg_sumsq_kernel, dim3(nch, nseg), dim3(256), 0, s, g, segs_dev, nch, part);
  OT_LAUNCH_CHECK("ot_clip_adam(sumsq)");
  hipLaunchKernelGGL(seg_scale_kernel, dim3(ceil_div(nseg, 256)), dim3(256), 0, s, part, segs_dev, nseg, nch, clip,
                     scale);
  OT_LAUNCH_CHECK("ot_clip_adam(scale)");
  hipLaunchKernelGGL(adam_kernel, dim3(nch, nseg), dim3(256), 0, s, w, g, m, v, segs_dev, scale, (float)alpha,
                     1.f - beta1, 1.f - beta2, eps, ptr_vec);
  OT_LAUNCH_CHECK("ot_clip_adam(apply)");
  return OT_OK;
}
