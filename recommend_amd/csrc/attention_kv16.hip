// Serving with a bf16 request cache (DESIGN.md §7b "Cache precision").
//
// The S-side K/V rows a request keeps between stage I and stage II are stored rounded to bf16 (round to nearest
// even, NaN stays NaN, past the bf16 range +-inf): half the resident bytes and half the bytes every (candidate,
// head) wave of stage II reads.  Rounding happens only when a row is stored:
//   ot_kv_pack_bf16          K | V columns of a span's f32 qkv rows -> the request's bf16 rows (one pass, in place
//                            at row0: the append of extend_requests writes behind the rows already there)
//   ot_attn_fwd_cached_kv16  attn_fwd_cached_kernel (attention_wave.hip) with the cached keys read as bf16 and widened
//                            in registers (bf16 -> f32 is a 16-bit shift, exact); a candidate's own rows stay f32,
//                            and the arithmetic is the f32 MFMA of the f32 kernel, so the result is the exact
//                            attention over [rounded cache ; f32 own rows] to f32 summation order.
// The f32 fragment helpers (acc_row, mm_frag, frag_to_lds, acc_tile_p, load_row_frag) are attn.h's, shared with the
// f32 kernels; only the bf16 row load is this file's.
#include "attn.h"

namespace ot {
namespace kv16 {

// load_row_frag's dims of a bf16 row: HD bytes as HD/16 16-byte loads, widened (element 2i the low half of dword i)
template <int HD>
__device__ __forceinline__ void load_row_frag16(float (&f)[HD / 2], const uint16_t* row, int hh) {
  const uint16_t* q = row + (HD / 2) * hh;
#pragma unroll
  for (int i = 0; i < HD / 16; ++i) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(q + 8 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[8 * i + 2 * k] = __uint_as_float(v[k] << 16);
      f[8 * i + 2 * k + 1] = __uint_as_float(v[k] & 0xffff0000u);
    }
  }
}

struct PackArgs {
  const float* qkv; int64_t ld;            // span rows [R*rows_per_req, ld]: q | k | v
  uint16_t* kv16; int64_t ldc16, req_stride, row0;
  int64_t rows_per_req, chunks;            // chunks = R * rows_per_req * (2d / 8)
  int d;
};

// one thread per 8 consecutive K | V columns of a row: two 16-byte loads, one 16-byte store (v_cvt_pk_bf16_f32)
__global__ __launch_bounds__(256) void kv_pack_bf16_kernel(PackArgs p) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.chunks) return;
  const int cpr = p.d / 4;                 // chunks per row
  const int64_t row = t / cpr;
  const int c = (int)(t - row * cpr);
  const int64_t r = row / p.rows_per_req, i = row - r * p.rows_per_req;
  const float* src = p.qkv + row * p.ld + p.d + 8 * c;
  const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
  const u32x2 lo = bf16_rne4(a), hi = bf16_rne4(b);
  *reinterpret_cast<u32x4*>(p.kv16 + (r * p.req_stride + p.row0 + i) * p.ldc16 + 8 * c) = u32x4{lo.x, lo.y, hi.x, hi.y};
}

struct AttnKv16Args {
  const float* qkv; int64_t ld;            // N-side rows [C*n, ld]: q | k | v
  const uint16_t* kv16; int64_t ldc16, req_stride;   // request r's cached key j: row r*req_stride + j, k | v bf16
  const int32_t* req;                      // [C] request of each candidate
  float* out;                              // [C*Kq, d]
  int C, H, Ic, n, Kq, d;
  float scale;
  float* lse;                              // [C, H, Kq] natural-log row statistics, or null
  const uint8_t* cache_valid; int64_t ldcv;          // the MASK instantiations only
};

// attn_fwd_cached_kernel<HD, MASK> with a per-lane key source of two formats: key < Ic a bf16 cache row, widened;
// key >= Ic the candidate's own f32 row.  A block that straddles Ic takes both branches once.
template <int HD, bool MASK>
__global__ __launch_bounds__(256) void attn_fwd_cached_kv16_kernel(AttnKv16Args p) {
  __shared__ __attribute__((aligned(16))) float lds[4][32 * TLD<HD>()];
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  float* tV = lds[threadIdx.x >> 6];
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= p.C * p.H) return;
  const int c = pair / p.H, h = pair % p.H;
  const int Ic = p.Ic, n = p.n, Kq = p.Kq, L = Ic + n;
  const int64_t r = p.req[c];
  const float* Nq = p.qkv + (int64_t)c * n * p.ld + h * HD;        // this candidate's N rows
  const int64_t c16 = r * p.req_stride * p.ldc16 + h * HD;         // element offset of the request's k, head h
  const int q_off = L - Kq;                                         // absolute position of query 0
  const float qscale = p.scale * 1.4426950408889634f;
  const int nqb = (Kq + 31) / 32;
  for (int qb = 0; qb < nqb; ++qb) {
    const int j = 32 * qb + li;
    const int qpos = q_off + (j < Kq ? j : Kq - 1);
    float qf[HD / 2];
    load_row_frag<HD>(qf, Nq + (int64_t)(qpos - Ic) * p.ld, hh);
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) qf[s] *= qscale;
    f32x16 oacc[NB(HD)];
#pragma unroll
    for (int cc = 0; cc < NB(HD); ++cc)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) oacc[cc][rr] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int last_q = q_off + min(32 * qb + 31, Kq - 1);
    const int nkb = last_q / 32 + 1;
    const int first_masked = (q_off + 32 * qb) / 32;
    for (int kb = 0; kb < nkb; ++kb) {
      const int key = 32 * kb + li;                 // this lane's key row (absolute position)
      float kf[HD / 2], vf[HD / 2];
      if (key < Ic) {
        const uint16_t* row = p.kv16 + c16 + (int64_t)key * p.ldc16;
        load_row_frag16<HD>(kf, row, hh);
        load_row_frag16<HD>(vf, row + p.d, hh);
      } else {
        const float* kr = key < L ? Nq + (int64_t)(key - Ic) * p.ld + p.d : nullptr;
        load_row_frag<HD>(kf, kr, hh);
        load_row_frag<HD>(vf, kr ? kr + p.d : nullptr, hh);
      }
      frag_to_lds<HD>(tV, vf, li, hh);
      f32x16 s = mm_frag<HD>(kf, qf);               // S^T (log2 units): row = key, col = query
      if constexpr (MASK) {
        const uint32_t vm = (uint32_t)__ballot(key < Ic ? p.cache_valid[r * p.ldcv + key] != 0 : key < L);
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const int kr = acc_row(rr, hh);
          s[rr] = (32 * kb + kr <= qpos && ((vm >> kr) & 1u)) ? s[rr] : -INFINITY;
        }
      } else if (kb >= first_masked) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) s[rr] = (32 * kb + acc_row(rr, hh) <= qpos) ? s[rr] : -INFINITY;
      }
      float mloc = s[0];
#pragma unroll
      for (int rr = 1; rr < 16; ++rr) mloc = fmaxf(mloc, s[rr]);
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
      const float mnew = fmaxf(m, mloc);
      const float msub = MASK && mnew == -INFINITY ? 0.f : mnew;   // MASK: no visible key yet
      const float corr = __builtin_amdgcn_exp2f(m - msub);
      float lsum = 0.f;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const float e = __builtin_amdgcn_exp2f(s[rr] - msub);
        s[rr] = e;
        lsum += e;
      }
      lsum += __shfl_xor(lsum, 32, 64);
      l = l * corr + lsum;
      m = mnew;
#pragma unroll
      for (int cc = 0; cc < NB(HD); ++cc) oacc[cc] *= corr;
      __builtin_amdgcn_wave_barrier();
      acc_tile_p<HD>(oacc, tV, s, li, hh);           // O^T += V^T P^T
      __builtin_amdgcn_wave_barrier();
    }
    if (j < Kq) {
      const float inv = 1.f / l;
      float* orow = p.out + ((int64_t)c * Kq + j) * p.d + h * HD;
#pragma unroll
      for (int cc = 0; cc < NB(HD); ++cc)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = 32 * cc + 8 * g + 4 * hh;
          if (dd < HD) {
            f32x4 v = {oacc[cc][4 * g] * inv, oacc[cc][4 * g + 1] * inv, oacc[cc][4 * g + 2] * inv,
                       oacc[cc][4 * g + 3] * inv};
            *reinterpret_cast<f32x4*>(orow + dd) = v;
          }
        }
      if (p.lse && hh == 0) p.lse[((int64_t)c * p.H + h) * Kq + j] = m * 0.6931471805599453f + __logf(l);
    }
  }
}

template <bool MASK>
static void launch_attn(const AttnKv16Args& p, int head_dim, hipStream_t st) {
  const dim3 grid(ceil_div((int64_t)p.C * p.H, 4));
  switch (head_dim) {
    case 16: hipLaunchKernelGGL((attn_fwd_cached_kv16_kernel<16, MASK>), grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL((attn_fwd_cached_kv16_kernel<32, MASK>), grid, dim3(256), 0, st, p); break;
    case 64: hipLaunchKernelGGL((attn_fwd_cached_kv16_kernel<64, MASK>), grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL((attn_fwd_cached_kv16_kernel<128, MASK>), grid, dim3(256), 0, st, p); break;
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace kv16
}  // namespace ot

using namespace ot;

extern "C" int ot_kv_pack_bf16(const float* qkv, int64_t ld, int R, int64_t rows_per_req, int d, uint16_t* kv16,
                               int64_t ldc16, int64_t req_stride, int64_t row0, void* stream) {
  OT_REQUIRE(R >= 0 && rows_per_req > 0 && d > 0 && d % 4 == 0 && row0 >= 0,
             "ot_kv_pack_bf16: bad sizes R=%d rows_per_req=%lld d=%d row0=%lld", R, (long long)rows_per_req, d,
             (long long)row0);
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * (int64_t)d, "ot_kv_pack_bf16: ld must hold q|k|v and be a multiple of 4");
  OT_REQUIRE(ldc16 % 8 == 0 && ldc16 >= 2 * (int64_t)d, "ot_kv_pack_bf16: ldc16 must hold k|v and be a multiple of 8");
  OT_REQUIRE(req_stride >= row0 + rows_per_req, "ot_kv_pack_bf16: req_stride %lld < row0 + rows_per_req = %lld",
             (long long)req_stride, (long long)(row0 + rows_per_req));
  OT_REQUIRE(qkv && kv16 && kv16::aligned16(qkv) && kv16::aligned16(kv16),
             "ot_kv_pack_bf16: null or not 16-byte aligned operand");
  if (R == 0) return OT_OK;
  const int64_t chunks = (int64_t)R * rows_per_req * (d / 4);
  OT_REQUIRE((chunks + 255) / 256 <= 0x7fffffffLL, "ot_kv_pack_bf16: grid too large");
  kv16::PackArgs p{qkv, ld, kv16, ldc16, req_stride, row0, rows_per_req, chunks, d};
  hipLaunchKernelGGL(kv16::kv_pack_bf16_kernel, dim3(ceil_div(chunks, 256)), dim3(256), 0, (hipStream_t)stream, p);
  OT_LAUNCH_CHECK("ot_kv_pack_bf16");
  return OT_OK;
}

extern "C" int ot_attn_fwd_cached_kv16(const float* qkv, int64_t ld, const uint16_t* kv16, int64_t ldc16,
                                       int64_t req_stride, const int32_t* req, int C, int H, int Ic, int n, int Kq,
                                       int head_dim, const uint8_t* cache_valid, int64_t ldcv, float* out,
                                       float* lse_or_null, void* stream) {
  OT_REQUIRE(C >= 0 && H > 0 && Ic >= 0 && n > 0 && Kq > 0 && Kq <= n,
             "ot_attn_fwd_cached_kv16: bad sizes C=%d Ic=%d n=%d Kq=%d", C, Ic, n, Kq);
  OT_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128,
             "ot_attn_fwd_cached_kv16: head_dim %d unsupported", head_dim);
  const int d = H * head_dim;
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * (int64_t)d, "ot_attn_fwd_cached_kv16: ld must hold q|k|v and be a multiple of 4");
  OT_REQUIRE(Ic == 0 || (ldc16 % 8 == 0 && ldc16 >= 2 * (int64_t)d),
             "ot_attn_fwd_cached_kv16: ldc16 must hold k|v and be a multiple of 8");
  OT_REQUIRE(Ic == 0 || req_stride >= Ic, "ot_attn_fwd_cached_kv16: req_stride %lld < Ic = %d", (long long)req_stride,
             Ic);
  OT_REQUIRE(qkv && out && req && (Ic == 0 || (kv16 && kv16::aligned16(kv16))) && kv16::aligned16(qkv) &&
                 kv16::aligned16(out),
             "ot_attn_fwd_cached_kv16: null or not 16-byte aligned operand");
  OT_REQUIRE(Ic == 0 || !cache_valid || ldcv >= Ic, "ot_attn_fwd_cached_kv16: ldcv < Ic");
  if (C == 0) return OT_OK;
  kv16::AttnKv16Args p{qkv, ld, kv16, ldc16, req_stride, req, out, C, H, Ic, n, Kq, d,
                       1.f / sqrtf((float)head_dim), lse_or_null, cache_valid, ldcv};
  if (cache_valid && Ic > 0) kv16::launch_attn<true>(p, head_dim, (hipStream_t)stream);
  else kv16::launch_attn<false>(p, head_dim, (hipStream_t)stream);
  OT_LAUNCH_CHECK("ot_attn_fwd_cached_kv16");
  return OT_OK;
}
