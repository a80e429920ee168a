// Micro-benchmark: cycles per MFMA gap of v_mfma_f32_32x32x16_f16 with VALU fillers behind each MFMA, per wave
// (s_memtime), at one and at two waves per SIMD (256-thread workgroups, one or two resident per CU), and the same
// filler streams with no MFMA in the loop.  Every instruction of the loop is inline asm, so the stream that runs is
// the stream written here.  Filler sets:
//   none
//   fma / mul / add   N = 2, 4, 6 scalar f32 instructions against N/2 packed ones (v_pk_*_f32), independent
//                     (every instruction its own register) and dependent (the scalar form as the two interleaved
//                     chains that one packed chain computes)
//   res_*             the fp16-pair residual l = fp16(x - f32(h)) of one element pair (common.h pair8 / pair4):
//                     pk    2 v_cvt_f32_f16 + v_pk_add_f32 + v_cvt_pk_f16_f32  (what a packed-f32 build emits)
//                     sub   2 v_cvt_f32_f16 + 2 v_sub_f32 + v_cvt_pk_f16_f32
//                     mix   2 v_fma_mix_f32 + v_cvt_pk_f16_f32
//                     mixlh v_fma_mixlo_f16 + v_fma_mixhi_f16
// The loop is bounded (a fixed trip count), no wave waits on another, and the only memory written is each wave's
// own two counters and one result per thread.
// Build: hipcc -O3 --offload-arch=gfx950 tools/valu_issue_bench.hip -o tools/valu_issue_bench
// Run:   tools/valu_issue_bench [out.md]      (valu_issue_bench.py builds it if needed and runs it)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

enum Op { NONE = 0, FMA, MUL, ADD, RES };
enum Form { SCALAR = 0, PACKED = 1, RES_PK = 0, RES_SUB = 1, RES_MIX = 2, RES_MIXLH = 3 };

#define CHECK(e)                                                                          \
  do {                                                                                    \
    hipError_t _e = (e);                                                                  \
    if (_e != hipSuccess) {                                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(_e));          \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

constexpr int GAPS = 8;        // MFMA gaps per loop iteration (4 accumulators in rotation)
constexpr int ITERS = 2000;    // loop trips: 16,000 gaps per wave and launch

// the fillers of one gap; s / p are the scalar and the packed working registers, c / d (ck / dk) the operands
template <int OP, int FORM, int N, bool DEP>
__device__ __forceinline__ void fillers(float (&s)[6], f32x2 (&p)[3], float c, float d, f32x2 ck, f32x2 dk, f32x2 x,
                                        unsigned h, unsigned& l) {
  if constexpr (OP == FMA || OP == MUL || OP == ADD) {
    if constexpr (FORM == SCALAR) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float& r = s[DEP ? (i & 1) : i];
        if constexpr (OP == FMA) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(r) : "v"(c), "v"(d));
        if constexpr (OP == MUL) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(r) : "v"(c));
        if constexpr (OP == ADD) asm volatile("v_add_f32 %0, %0, %1" : "+v"(r) : "v"(d));
      }
    } else {
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        f32x2& r = p[DEP ? 0 : i];
        if constexpr (OP == FMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(r) : "v"(ck), "v"(dk));
        if constexpr (OP == MUL) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(r) : "v"(ck));
        if constexpr (OP == ADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(r) : "v"(dk));
      }
    }
  } else if constexpr (OP == RES) {
    if constexpr (FORM == RES_PK || FORM == RES_SUB) {
      f32x2 t;
      asm volatile(
          "v_cvt_f32_f16_e32 %0, %2\n\t"
          "v_cvt_f32_f16_sdwa %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1"
          : "=&v"(t.x), "=&v"(t.y)
          : "v"(h));
      if constexpr (FORM == RES_PK) {
        asm volatile("v_pk_add_f32 %0, %1, %0 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(t) : "v"(x));
      } else {
        asm volatile(
            "v_sub_f32_e32 %0, %2, %0\n\t"
            "v_sub_f32_e32 %1, %3, %1"
            : "+v"(t.x), "+v"(t.y)
            : "v"(x.x), "v"(x.y));
      }
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(l) : "v"(t.x), "v"(t.y));
    } else if constexpr (FORM == RES_MIX) {
      float t0, t1;
      asm volatile(
          "v_fma_mix_f32 %0, %2, 1.0, -%4 op_sel_hi:[0,0,1]\n\t"
          "v_fma_mix_f32 %1, %3, 1.0, -%4 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
          : "=&v"(t0), "=&v"(t1)
          : "v"(x.x), "v"(x.y), "v"(h));
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(l) : "v"(t0), "v"(t1));
    } else {
      asm volatile(
          "v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel_hi:[0,0,1]\n\t"
          "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
          : "=&v"(l)
          : "v"(x.x), "v"(x.y), "v"(h));
    }
  }
}

// LDS_BYTES sets how many 256-thread workgroups fit a CU (160 KiB of LDS): 96 KiB one, 64 KiB two
template <int OP, int FORM, int N, bool DEP, bool MFMA, int LDS_BYTES>
__global__ __launch_bounds__(256) void kern(float* out, long long* stamps, int iters) {
  __shared__ float lds[LDS_BYTES / 4];
  lds[threadIdx.x] = 1.f + threadIdx.x;
  __syncthreads();
  f32x16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  const unsigned one2 = 0x3c003c00u;   // fp16 {1, 1}
  u32x4 fa = {one2, one2, one2, one2}, fb = {one2 ^ (threadIdx.x & 1u) << 15, one2, one2, one2};
  float s[6];
  f32x2 p[3];
#pragma unroll
  for (int i = 0; i < 6; ++i) s[i] = 1.f + 0.001f * (float)(threadIdx.x + i);
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = f32x2{s[2 * i], s[2 * i + 1]};
  // the working values stay finite: fma x <- 0.5 x + 1, mul x <- x * 1, add x <- x + 0
  const float c = OP == FMA ? 0.5f : 1.f, d = OP == FMA ? 1.f : 0.f;
  const f32x2 ck = {c, c}, dk = {d, d};
  const f32x2 x = {1.0009765f + 1e-6f * (float)threadIdx.x, -3.0004883f};
  unsigned h, l = 0;
  asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h) : "v"(x.x), "v"(x.y));
  const long long t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int g = 0; g < GAPS; ++g) {
      if constexpr (MFMA)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc[g & 3]) : "v"(fa), "v"(fb));
      fillers<OP, FORM, N, DEP>(s, p, c, d, ck, dk, x, h, l);
    }
  }
  // the last MFMAs retire before compiler-generated code reads their accumulators
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  const long long t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float r = lds[(threadIdx.x * 7) & 255] + __uint_as_float(l);
#pragma unroll
  for (int i = 0; i < 6; ++i) r += s[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) r += p[i].x + p[i].y;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int k = 0; k < 16; ++k) r += acc[a][k];
  out[(size_t)blockIdx.x * 256 + threadIdx.x] = r;
  if ((threadIdx.x & 63) == 0) {
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    stamps[2 * w] = t0;
    stamps[2 * w + 1] = t1;
  }
}

struct Result { double med, lo; };

static int g_cus = 0;
static float* g_out = nullptr;
static long long* g_stamps = nullptr;

template <int OP, int FORM, int N, bool DEP, bool MFMA, int LDS_BYTES>
static Result launch(int wgs_per_cu) {
  const int blocks = g_cus * wgs_per_cu;
  CHECK(hipMemset(g_stamps, 0, (size_t)blocks * 8 * sizeof(long long)));
  for (int rep = 0; rep < 2; ++rep)   // the first launch loads the code object and warms the clock
    hipLaunchKernelGGL((kern<OP, FORM, N, DEP, MFMA, LDS_BYTES>), dim3(blocks), dim3(256), 0, 0, g_out, g_stamps, ITERS);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<long long> h((size_t)blocks * 8);
  CHECK(hipMemcpy(h.data(), g_stamps, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
  std::vector<double> cyc;
  for (size_t w = 0; w < (size_t)blocks * 4; ++w) cyc.push_back((double)(h[2 * w + 1] - h[2 * w]) / (ITERS * GAPS));
  std::sort(cyc.begin(), cyc.end());
  return Result{cyc[cyc.size() / 2], cyc[0]};
}

static std::string g_table;

template <int OP, int FORM, int N, bool DEP>
static void row(const char* name) {
  const Result a = launch<OP, FORM, N, DEP, true, 96 * 1024>(1), b = launch<OP, FORM, N, DEP, true, 64 * 1024>(2);
  const Result e = launch<OP, FORM, N, DEP, false, 96 * 1024>(1), f = launch<OP, FORM, N, DEP, false, 64 * 1024>(2);
  char buf[256];
  snprintf(buf, sizeof buf, "| %-22s | %6.1f | %6.1f | %6.1f | %6.1f | %6.1f | %6.1f |\n", name, a.med, a.lo, b.med, b.lo,
           e.med, f.med);
  g_table += buf;
  fputs(buf, stdout);
  fflush(stdout);
}

template <int OP>
static void op_rows(const char* op) {
  char n[64];
#define ROWS(N)                                                                  \
  snprintf(n, sizeof n, "%d v_%s_f32", N, op);          row<OP, SCALAR, N, false>(n); \
  snprintf(n, sizeof n, "%d v_pk_%s_f32", N / 2, op);   row<OP, PACKED, N, false>(n); \
  snprintf(n, sizeof n, "%d v_%s_f32 dep", N, op);      row<OP, SCALAR, N, true>(n);  \
  snprintf(n, sizeof n, "%d v_pk_%s_f32 dep", N / 2, op); row<OP, PACKED, N, true>(n);
  ROWS(2) ROWS(4) ROWS(6)
#undef ROWS
}

int main(int argc, char** argv) {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  g_cus = prop.multiProcessorCount;
  CHECK(hipMalloc(&g_out, (size_t)g_cus * 2 * 256 * sizeof(float)));
  CHECK(hipMalloc(&g_stamps, (size_t)g_cus * 2 * 8 * sizeof(long long)));
  char head[512];
  snprintf(head, sizeof head,
           "%s, %d CUs; cycles (s_memtime) per gap and wave, %d gaps per wave; 1w / 2w = waves per SIMD "
           "(one / two 256-thread workgroups per CU)\n\n"
           "| fillers per gap | MFMA 1w med | 1w min | MFMA 2w med | 2w min | no MFMA 1w med | no MFMA 2w med |\n"
           "|---|---|---|---|---|---|---|\n",
           prop.gcnArchName, g_cus, ITERS * GAPS);
  g_table = head;
  fputs(head, stdout);
  row<NONE, 0, 0, false>("none");
  op_rows<FMA>("fma");
  op_rows<MUL>("mul");
  op_rows<ADD>("add");
  row<RES, RES_PK, 0, false>("res_pk (cvt,cvt,pk_add,cvt_pk)");
  row<RES, RES_SUB, 0, false>("res_sub (cvt,cvt,sub,sub,cvt_pk)");
  row<RES, RES_MIX, 0, false>("res_mix (mix,mix,cvt_pk)");
  row<RES, RES_MIXLH, 0, false>("res_mixlh (mixlo,mixhi)");
  if (argc > 1) {
    FILE* f = fopen(argv[1], "w");
    if (!f) { perror(argv[1]); return 1; }
    fputs(g_table.c_str(), f);
    fclose(f);
  }
  CHECK(hipFree(g_out));
  CHECK(hipFree(g_stamps));
  return 0;
}
