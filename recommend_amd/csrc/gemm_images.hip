// The pre-split weight images the plane GEMMs (gemm_plane.hip, gemm_plane_wide.hip) copy into LDS: ot_split_images.
#include <atomic>
#include <cstdlib>

#include "gemm.h"

namespace ot {

// Pre-split B images (ot_split_images).  desc [nd][10] int64: {src_off, sn, sk, gstride, kscale_off
// (-1: none), dst_off (ushorts), first_unit, G, N, K}; B[g][n][k] = src[g*gstride + n*sn + k*sk]
// (* kscale[k]); one unit = one (g, n tile, 16-k stage) block of 3 x 128 x 16 16-bit planes, one thread per
// (row n, 8-k half), each plane's 16 B at its swizzled half.  Split mode: the exact three-plane bf16 split (split8),
// except for gamma-folded images (kscale_off >= 0: the RMSNorm-prologue GEMMs, plane_gemm_kernel TERMS 2): the
// scaled fp16 pair (planes 0, 1) of B[g][n][k] s_n, s_n a power of two per column n (image_colscale_kernel, stored
// as 128 floats in plane 2 of the tile's first unit); bf16 mode: plane 0 = the value rounded to nearest.
__device__ __forceinline__ const int64_t* image_unit(const int64_t* desc, int nd, int64_t unit, int64_t& g, int64_t& tn,
                                                     int64_t& ks) {
  int b = 0;
  while (b + 1 < nd && desc[10 * (b + 1) + 6] <= unit) ++b;
  const int64_t* d = desc + 10 * b;
  const int64_t G = d[7], N = d[8], K = d[9];
  const int64_t ntn = (N + GT - 1) / GT, nks = K / 16;
  int64_t u = unit - d[6];
  if (u >= G * ntn * nks) return nullptr;
  g = u / (ntn * nks);
  u %= ntn * nks;
  tn = u / nks;
  ks = u % nks;
  return d;
}

// per column n of each (group, n tile): the power-of-two scale putting max_k |B[g][n][k]| in [2^13, 2^14) (one
// block per image unit; the tile's first-unit blocks work, two threads per column)
__global__ __launch_bounds__(256) void image_colscale_kernel(const float* __restrict__ base, const int64_t* __restrict__ desc,
                                                             int nd, uint16_t* img) {
  int64_t g, tn, ks;
  const int64_t* d = image_unit(desc, nd, blockIdx.x, g, tn, ks);
  if (!d || ks != 0 || d[4] == -1) return;
  const int64_t N = d[8], K = d[9];
  const int n = threadIdx.x >> 1, hh = threadIdx.x & 1;
  const int64_t gn = tn * GT + n;
  float m = 0.f;
  if (gn < N) {
    const float* src = base + d[0] + g * d[3] + gn * d[1];
#pragma unroll 8
    for (int64_t k = hh; k < K; k += 2) {
      float x = src[k * d[2]];
      if (d[4] >= 0) x *= base[d[4] + k];
      m = fmaxf(m, fabsf(x));
    }
  }
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  float* csc = reinterpret_cast<float*>(img + d[5] + ((int64_t)blockIdx.x - d[6]) * (PG_B_BYTES / 2) + 2 * GT * 16);
  if (hh == 0) csc[n] = pow2_scale14(m);
  if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(csc)[GT] = PAIR_IMAGE_TAG;   // the form tag (see PAIR_IMAGE_TAG)
}

__global__ __launch_bounds__(256) void split_images_kernel(const float* __restrict__ base, const int64_t* __restrict__ desc,
                                                           int nd, uint16_t* img, int one) {
  const int64_t unit = blockIdx.x;
  int64_t g, tn, ks;
  const int64_t* d = image_unit(desc, nd, unit, g, tn, ks);
  if (!d) return;
  const int64_t N = d[8];
  const int n = threadIdx.x >> 1, hh = threadIdx.x & 1;
  const int64_t gn = tn * GT + n;
  const float* src = base + d[0] + g * d[3] + gn * d[1];
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t k = ks * 16 + 8 * hh + j;
    float x = gn < N ? src[k * d[2]] : 0.f;
    if (d[4] >= 0) x *= base[d[4] + k];
    v[j] = x;
  }
  uint16_t* dst = img + d[5] + (unit - d[6]) * (PG_B_BYTES / 2);
  u32x4 pl[3];
  const bool pair = !one && d[4] != -1;                 // gamma-folded (>= 0) or the -2 pair form
  if (one) {
    split8t<1>(v, pl);                                // OT_MATMUL_BF16: plane 0 = round to nearest
  } else if (pair) {
    const float sn = reinterpret_cast<const float*>(dst - ks * (PG_B_BYTES / 2) + 2 * GT * 16)[n];
    pair8(v, sn, pl);
  } else {
    split8(v, pl);
  }
  const int npl = one ? 1 : pair ? 2 : 3;            // (pair: plane 2 of the first unit holds the column scales)
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (q < npl) *reinterpret_cast<u32x4*>(dst + q * GT * 16 + n * 16 + 8 * (hh ^ ((n >> 3) & 1))) = pl[q];
}

// ---- the one-launch build (ot_image_build 1) ---------------------------------------------------------------------
// One workgroup per (descriptor, g, column tile), walked by a grid of at most IMG_GRID_PER_CU workgroups per compute
// unit: the tile's workgroup takes the 128 column maxima over the whole K with all 256 threads (pair forms only),
// keeps each scale in the register of the thread that needs it, then sweeps K a second time, out of the caches, to
// split and store the tile's K / 16 units.  The bytes are those of image_colscale_kernel + split_images_kernel: the
// maximum is order-free and every element goes through the same pair8 / split8 / split8t<1>.
// The tile is found without touching first_unit: every workgroup reads the descriptors' G and N once (one coalesced
// load), scans the tiles per descriptor in LDS and finds its descriptor by a binary search of that scan; a bank's
// units are consecutive from its first_unit, so a tile's units past total_units are left out as the one-block-per-unit
// kernels leave them out.
constexpr int IMG_MAXD = 256;          // descriptors per launch the LDS scan holds (more: the two-kernel build runs)
constexpr int IMG_GRID_PER_CU = 3;          // C2 has 753 tiles: one each on 768 workgroups; T's 1,508 two each

// the 8 values of thread (n, 8-k half) for the stage at k0: B[g][n][k0 + j] (* kscale[k0 + j]); VK: k contiguous and
// 16-B aligned, two float4 loads per operand
template <bool VK>
__device__ __forceinline__ void image_load8(const float* __restrict__ row, bool live, int64_t sk,
                                            const float* __restrict__ ksc, int64_t k0, float (&v)[8]) {
  if constexpr (VK) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (live) {
      a = *reinterpret_cast<const f32x4*>(row + k0);
      b = *reinterpret_cast<const f32x4*>(row + k0 + 4);
    }
    if (ksc) {
      a *= *reinterpret_cast<const f32x4*>(ksc + k0);
      b *= *reinterpret_cast<const f32x4*>(ksc + k0 + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j], v[4 + j] = b[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = live ? row[(k0 + j) * sk] : 0.f;
      if (ksc) x *= ksc[k0 + j];
      v[j] = x;
    }
  }
}

// max_k |B[g][n][k]| of thread (n, half)'s own k, the two halves combined
template <bool VK>
__device__ __forceinline__ float image_colmax(const float* __restrict__ row, bool live, int64_t sk,
                                              const float* __restrict__ ksc, int hh, int nks) {
  float m = 0.f;
  if (live) {
#pragma unroll 4
    for (int ks = 0; ks < nks; ++ks) {
      float v[8];
      image_load8<VK>(row, true, sk, ksc, ks * 16 + 8 * hh, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
    }
  }
  return fmaxf(m, __shfl_xor(m, 1, 64));
}

template <bool VK>
__device__ __forceinline__ void image_split_units(const float* __restrict__ row, bool live, int64_t sk,
                                                  const float* __restrict__ ksc, int n, int hh, int nks, int form,
                                                  float scale, uint16_t* dst) {
  uint16_t* out = dst + n * 16 + 8 * (hh ^ ((n >> 3) & 1));
#pragma unroll 2
  for (int ks = 0; ks < nks; ++ks, out += PG_B_BYTES / 2) {
    float v[8];
    image_load8<VK>(row, live, sk, ksc, ks * 16 + 8 * hh, v);
    u32x4 pl[3];
    if (form == 1) {                                   // OT_MATMUL_BF16: plane 0 = round to nearest
      split8t<1>(v, pl);
      *reinterpret_cast<u32x4*>(out) = pl[0];
    } else if (form == 2) {                            // pair (plane 2 of the first unit holds the column scales)
      pair8(v, scale, pl);
      *reinterpret_cast<u32x4*>(out) = pl[0];
      *reinterpret_cast<u32x4*>(out + GT * 16) = pl[1];
    } else {
      split8(v, pl);
#pragma unroll
      for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(out + q * GT * 16) = pl[q];
    }
  }
}

__global__ __launch_bounds__(256) void build_images_kernel(const float* __restrict__ base, const int64_t* __restrict__ desc,
                                                           int nd, int64_t total_units, uint16_t* img, int one) {
  __shared__ int tiles[IMG_MAXD];           // inclusive scan of the tiles per descriptor
  __shared__ float part[8][GT];             // n-contiguous maxima: the partial maxima of the 8 k residues
  const int tid = threadIdx.x;
  {
    int c = 0;
    if (tid < nd) c = (int)(desc[10 * tid + 7] * ((desc[10 * tid + 8] + GT - 1) / GT));
    tiles[tid] = c;
    __syncthreads();
    for (int o = 1; o < IMG_MAXD; o <<= 1) {
      const int a = tid >= o ? tiles[tid - o] : 0;
      __syncthreads();
      tiles[tid] += a;
      __syncthreads();
    }
  }
  const int ntiles = tiles[IMG_MAXD - 1];
  const int n = tid >> 1, hh = tid & 1;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int lo = 0, hi = nd - 1;                 // the first descriptor whose scan exceeds t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tiles[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int64_t* d = desc + 10 * lo;
    const int64_t sn = d[1], sk = d[2], kso = d[4], N = d[8], K = d[9];
    const int ntn = (int)((N + GT - 1) / GT), nks_all = (int)(K / 16);
    const int local = t - (lo ? tiles[lo - 1] : 0), g = local / ntn, tn = local % ntn;
    const int64_t u0 = (int64_t)local * nks_all;                       // the tile's first unit within its bank
    const int64_t left = total_units - (d[6] + u0);
    if (left <= 0) continue;
    const int nks = left < nks_all ? (int)left : nks_all;
    const int64_t so = d[0] + g * d[3];
    const float* src = base + so;
    const float* ksc = kso >= 0 ? base + kso : nullptr;
    const int form = one ? 1 : kso != -1 ? 2 : 0;
    uint16_t* dst = img + d[5] + u0 * (PG_B_BYTES / 2);
    const int64_t gn = (int64_t)tn * GT + n;
    const bool live = gn < N;
    const float* row = src + gn * sn;
    // 16-byte loads along the contiguous axis where the strides and offsets keep them aligned
    const bool al = (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (so & 3) == 0;
    const bool vk = al && sk == 1 && (sn & 3) == 0 && (kso < 0 || (kso & 3) == 0);
    const bool vn = al && sn == 1 && (sk & 3) == 0 && (N & 3) == 0;
    float scale = 1.f;
    if (form == 2) {
      float m;
      if (vk) {
        m = image_colmax<true>(row, live, sk, ksc, hh, nks_all);
      } else if (vn) {
        // thread (k residue r, column quad c): a float4 of four columns per k, 512-B runs per k row
        const int r = tid >> 5, c = tid & 31;
        f32x4 m4 = {0.f, 0.f, 0.f, 0.f};
        if ((int64_t)tn * GT + 4 * c < N) {
          const float* p = src + (int64_t)tn * GT + 4 * c;
#pragma unroll 4
          for (int64_t k = r; k < K; k += 8) {
            f32x4 x = *reinterpret_cast<const f32x4*>(p + k * sk);
            if (ksc) x *= ksc[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) m4[j] = fmaxf(m4[j], fabsf(x[j]));
          }
        }
        *reinterpret_cast<f32x4*>(&part[r][4 * c]) = m4;
        __syncthreads();
        m = part[0][n];
#pragma unroll
        for (int q = 1; q < 8; ++q) m = fmaxf(m, part[q][n]);
        __syncthreads();
      } else {
        m = image_colmax<false>(row, live, sk, ksc, hh, nks_all);
      }
      scale = pow2_scale14(m);
      float* csc = reinterpret_cast<float*>(dst + 2 * GT * 16);
      if (hh == 0) csc[n] = scale;
      if (tid == 0) reinterpret_cast<uint32_t*>(csc)[GT] = PAIR_IMAGE_TAG;   // the form tag (see PAIR_IMAGE_TAG)
    }
    if (vk) image_split_units<true>(row, live, sk, ksc, n, hh, nks, form, scale, dst);
    else image_split_units<false>(row, live, sk, ksc, n, hh, nks, form, scale, dst);
  }
}

// 1 = ot_split_images is the one-launch build (build_images_kernel), 0 = image_colscale_kernel + split_images_kernel,
// the reference path of tests/test_image_build_gpu.py; the environment variable ONETRANS_IMAGE_BUILD (0 / 1) sets the
// process's initial value
#ifndef OT_IMAGE_BUILD
#define OT_IMAGE_BUILD 1
#endif
static int image_build_initial() {
  const char* e = getenv("ONETRANS_IMAGE_BUILD");
  return e && *e ? (atoi(e) != 0) : OT_IMAGE_BUILD;
}
static std::atomic<int> g_image_build{image_build_initial()};

static int image_grid_cap() {
  static const int cap = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return IMG_GRID_PER_CU * cus;
  }();
  return cap;
}

}  // namespace ot

using namespace ot;

extern "C" int ot_image_build(int on) {
  const int old = g_image_build.load(std::memory_order_relaxed);
  if (on >= 0) g_image_build.store(on ? 1 : 0, std::memory_order_relaxed);
  return old;
}

extern "C" size_t ot_split_image_elems(int G, int N, int K) {
  if (G <= 0 || N <= 0 || K <= 0 || K % 16) return 0;
  return (size_t)G * ceil_div(N, GT) * (K / 16) * (PG_B_BYTES / 2);
}

extern "C" int ot_split_images(const float* base, const int64_t* desc_dev, int ndesc, int64_t total_units,
                               uint16_t* img, int precision, void* stream) {
  OT_REQUIRE(base && desc_dev && img && ndesc > 0 && total_units >= 0, "ot_split_images: bad args");
  OT_REQUIRE(precision == OT_MATMUL_SPLIT_BF16 || precision == OT_MATMUL_BF16,
             "ot_split_images: precision %d has no plane images", precision);
  if (total_units == 0) return OT_OK;
  OT_REQUIRE(total_units <= 0x7fffffff, "ot_split_images: %lld units", (long long)total_units);
  if (g_image_build.load(std::memory_order_relaxed) && ndesc <= IMG_MAXD) {
    // the tile count is on the device only; a tile has K / 16 units, so total_units bounds it from above, and past
    // IMG_GRID_PER_CU workgroups per compute unit the workgroups walk several tiles each
    const int64_t cap = image_grid_cap();
    hipLaunchKernelGGL(build_images_kernel, dim3((unsigned)(total_units < cap ? total_units : cap)), dim3(256), 0,
                       (hipStream_t)stream, base, desc_dev, ndesc, total_units, img, precision == OT_MATMUL_BF16 ? 1 : 0);
    OT_LAUNCH_CHECK("ot_split_images(build)");
    return OT_OK;
  }
  if (precision == OT_MATMUL_SPLIT_BF16) {
    hipLaunchKernelGGL(image_colscale_kernel, dim3((unsigned)total_units), dim3(256), 0, (hipStream_t)stream, base,
                       desc_dev, ndesc, img);
    OT_LAUNCH_CHECK("ot_split_images(column scales)");
  }
  hipLaunchKernelGGL(split_images_kernel, dim3((unsigned)total_units), dim3(256), 0, (hipStream_t)stream, base,
                     desc_dev, ndesc, img, precision == OT_MATMUL_BF16 ? 1 : 0);
  OT_LAUNCH_CHECK("ot_split_images");
  return OT_OK;
}
