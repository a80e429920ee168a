// Probe of the scaled fp16-pair split (common.h pair8 / pair4): the two fp16 planes of a flat f32 vector, written
// out so a test can compare them bit for bit with the definition (tests/test_pair_split_gpu.py).  Not on any hot
// path.  Each form is compiled as its users are (Makefile SCALAR_F32_SRCS): pair8 with packed f32 like the plane
// GEMMs and the fused FFN, pair4 without it like gemm_wgrad.hip (OT_SCALAR_F32 below is that flag for one kernel).
#include "common.h"

namespace ot {

#if defined(__HIP_DEVICE_COMPILE__)
#define OT_SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define OT_SCALAR_F32   // the host pass knows no such feature
#endif
// FORM 0: pair8 (8 elements per thread, the scale and the saturation inside); FORM 1: pair4 of x * scale (the
// weight gradient's use: 4 elements per thread, no saturation); FORM 2: the slice attention's split of x * scale
// (attention_slice.hip splitN<2>: no saturation, the residual by pair_lo_mix)
template <int FORM>
__device__ __forceinline__ void pair_probe_body(const float* __restrict__ x, int64_t ngroups, float scale,
                                                uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;
  if constexpr (FORM == 0) {
    float v[8];
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + g * 8), b = *reinterpret_cast<const f32x4*>(x + g * 8 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    u32x4 pl[3];
    pair8(v, scale, pl);
    *reinterpret_cast<u32x4*>(hi + g * 8) = pl[0];
    *reinterpret_cast<u32x4*>(lo + g * 8) = pl[1];
  } else if constexpr (FORM == 2) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + g * 4);
    const f32x2_t x0 = f32x2_t{a.x, a.y} * scale, x1 = f32x2_t{a.z, a.w} * scale;
    const f16x2_t h0 = __builtin_convertvector(x0, f16x2_t), h1 = __builtin_convertvector(x1, f16x2_t);
    const f16x2_t l0 = pair_lo_mix(x0, h0), l1 = pair_lo_mix(x1, h1);
    *reinterpret_cast<u32x2*>(hi + g * 4) = u32x2{__builtin_bit_cast(uint32_t, h0), __builtin_bit_cast(uint32_t, h1)};
    *reinterpret_cast<u32x2*>(lo + g * 4) = u32x2{__builtin_bit_cast(uint32_t, l0), __builtin_bit_cast(uint32_t, l1)};
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + g * 4);
    u32x2 h, l;
    pair4(a * scale, h, l);
    *reinterpret_cast<u32x2*>(hi + g * 4) = h;
    *reinterpret_cast<u32x2*>(lo + g * 4) = l;
  }
}
__global__ __launch_bounds__(256) void pair8_probe_kernel(const float* x, int64_t ngroups, float scale, uint16_t* hi,
                                                          uint16_t* lo) {
  pair_probe_body<0>(x, ngroups, scale, hi, lo);
}
__global__ __launch_bounds__(256) OT_SCALAR_F32 void pair4_probe_kernel(const float* x, int64_t ngroups, float scale,
                                                                        uint16_t* hi, uint16_t* lo) {
  pair_probe_body<1>(x, ngroups, scale, hi, lo);
}
__global__ __launch_bounds__(256) OT_SCALAR_F32 void slice_probe_kernel(const float* x, int64_t ngroups, float scale,
                                                                        uint16_t* hi, uint16_t* lo) {
  pair_probe_body<2>(x, ngroups, scale, hi, lo);
}

}  // namespace ot

extern "C" int ot_pair_split_probe(const float* x, int64_t n, float scale, int form, uint16_t* hi, uint16_t* lo,
                                   void* stream) {
  using namespace ot;
  OT_REQUIRE(x && hi && lo, "ot_pair_split_probe: null operand");
  OT_REQUIRE(form >= 0 && form <= 2, "ot_pair_split_probe: form is 0 (pair8), 1 (pair4) or 2 (slice split)");
  const int per = form == 0 ? 8 : 4;
  OT_REQUIRE(n >= 0 && n % per == 0 && n / per <= ((int64_t)1 << 31) - 256,
             "ot_pair_split_probe: n must be a multiple of %d", per);
  OT_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)hi % 16) == 0 && ((uintptr_t)lo % 16) == 0,
             "ot_pair_split_probe: x / hi / lo must be 16-byte aligned");
  if (n == 0) return OT_OK;
  const int64_t groups = n / per;
  if (form == 0)
    hipLaunchKernelGGL(pair8_probe_kernel, dim3(ceil_div(groups, 256)), dim3(256), 0, (hipStream_t)stream, x, groups,
                       scale, hi, lo);
  else if (form == 2)
    hipLaunchKernelGGL(slice_probe_kernel, dim3(ceil_div(groups, 256)), dim3(256), 0, (hipStream_t)stream, x, groups,
                       scale, hi, lo);
  else
    hipLaunchKernelGGL(pair4_probe_kernel, dim3(ceil_div(groups, 256)), dim3(256), 0, (hipStream_t)stream, x, groups,
                       scale, hi, lo);
  OT_LAUNCH_CHECK("ot_pair_split_probe");
  return OT_OK;
}
