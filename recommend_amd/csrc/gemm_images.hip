// The pre-split weight images the plane GEMMs (gemm_plane.hip, gemm_plane_wide.hip) copy into LDS: ot_split_images.
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

}  // namespace ot

using namespace ot;

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
