// The last layer's attention with one query per sample (Kq = 1), folded through the shared-weight K / V projection
// (C-ABI: ot_attn_fold_* in include/onetrans_hip.h; the algebra: DESIGN.md §5, tests/fold_ref.py).
//
// For the keys j of weight group 0 (S) the projected key is K_j = Wk0^T (gamma o xh_j), xh_j = x_j rstd_j, so the
// score against the one query q_h is <xh_j, qt_h> with the folded query qt_h = gamma o (Wk0[:, h] q_h), and the
// value sum is Wv0[:, h]^T (gamma o y_h), y_h = sum_j p_h[j] xh_j.  The keys of the dedicated groups (D) keep their
// projected K / V rows (read from qkv).  The forward streams a sample's rows once; the backward streams them once
// more and writes dx (norm backward applied) for the S rows, dK / dV / dq for the D rows and the query, and
// z_h = sum_j ds_h[j] xh_j, from which the group-0 weight gradients are dWk0[:, h] = (gamma o z_h) q_h^T,
// dWv0[:, h] = (gamma o y_h) do_h^T (ot_attn_fold_dw: per-chunk partials summed in a fixed order).
//
// Plain f32 FMA.  One workgroup of 256 threads per sample; a half-wave (32 lanes x float4) holds one row of 128
// floats, so a wave works on two rows at a time and eight rows are in flight per workgroup; the eight half-waves'
// online-softmax states are merged through LDS in a fixed order (results are run-to-run bit-identical).
#include <atomic>
#include <cstdlib>

#include "gemm.h"      // half_sum follows its row32_max

namespace ot {
namespace fold {

constexpr int FD = 128;          // row width: 32 lanes x float4
constexpr int NHW = 8;           // half-waves (rows in flight) per workgroup
constexpr int DW_ROWS = 32;      // samples per partial of the weight gradient

struct FoldArgs {
  const float* x; int64_t ldx; const float* rstd; const float* gamma;
  const float* w; int64_t ldw;          // group 0's Wqkv [d][3d]: Wk at column d, Wv at column 2d
  const float* wT; int64_t ldwT;        // its transpose [3d][d]
  const float* qkv; int64_t ldqkv;      // rows b*I + p: q of the query row, K / V of the dedicated rows
  int B, I, ded0, ded1; float scale;    // positions ded0 <= p < ded1 are the dedicated keys
  float* o; float* lse; float* y;       // forward outputs, backward inputs
  const float* dout; const float* dx1;
  float* dx; int64_t lddx; float* dqkv; int64_t lddqkv; int nf; float* z; float* dgpart;
};

// sum over the 32 lanes that hold one row, every lane receiving the same bits: gemm.h's row32_max with adds (quad
// swaps, half-row and row mirrors by DPP, then the two 16-lane rows by v_permlane16_swap) — VALU only.  The shuffle
// form (row32_sum: five ds_bpermute round trips) measured 150 / 286 us for the C2 forward / backward launches, LDS-issue
// bound: the backward makes nine such sums per row.
__device__ __forceinline__ float half_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));    // quad [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));    // quad [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));   // row_mirror
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// out[h][k] = sum_c wT[(col0 + h HD + c)][k] v[h HD + c]: the [d x hd] block of head h times that head's vector
template <int H>
__device__ __forceinline__ void head_matvec_T(const float* wT, int64_t ldwT, int col0, const float* v,
                                              float (*out)[FD], int t) {
  constexpr int HD = FD / H;
  for (int idx = t; idx < H * FD; idx += 256) {
    const int h = idx / FD, k = idx % FD;
    const float* wk = wT + (int64_t)(col0 + h * HD) * ldwT + k;
    float a = 0.f;
#pragma unroll 8
    for (int c = 0; c < HD; ++c) a = fmaf(wk[(int64_t)c * ldwT], v[h * HD + c], a);
    out[h][k] = a;
  }
}

// part[half][n] = sum over k in this half of w[k][col0 + n] gv[head(n)][k]  (n = t & 127, half = t >> 7)
template <int H>
__device__ __forceinline__ void head_matvec(const float* w, int64_t ldw, int col0, const float (*gv)[FD],
                                            float (*part)[FD], int t) {
  constexpr int HD = FD / H;
  const int n = t & (FD - 1), half = t >> 7, h = n / HD;
  const float* wn = w + (int64_t)(half * 64) * ldw + col0 + n;
  float a = 0.f;
#pragma unroll 8
  for (int k = 0; k < 64; ++k) a = fmaf(wn[(int64_t)k * ldw], gv[h][half * 64 + k], a);
  part[half][n] = a;
}

template <int H>
__global__ __launch_bounds__(256) void attn_fold_fwd_kernel(FoldArgs p) {
  constexpr int HD = FD / H, LPH = 32 / H;       // lanes of a half-wave per head
  __shared__ __attribute__((aligned(16))) float qs[FD];
  __shared__ __attribute__((aligned(16))) float qt[H][FD];
  __shared__ float rm[NHW][H], rl[NHW][H];
  __shared__ __attribute__((aligned(16))) float ry[NHW][H][FD];
  __shared__ __attribute__((aligned(16))) float ro[NHW][FD];
  __shared__ float gy[H][FD];
  __shared__ float po[2][FD];
  const int b = blockIdx.x, t = threadIdx.x, hw = t >> 5, lane = t & 31, myh = lane / LPH;
  const int64_t row0 = (int64_t)b * p.I;
  if (t < FD) qs[t] = p.qkv[(row0 + p.I - 1) * p.ldqkv + t];
  __syncthreads();
  head_matvec_T<H>(p.wT, p.ldwT, FD, qs, qt, t);
  __syncthreads();
  const f32x4 gam = ld4(p.gamma + 4 * lane);
  const f32x4 q4 = ld4(qs + 4 * lane);
  f32x4 qth[H], yv[H];
  float m[H], l[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    qth[h] = ld4(&qt[h][4 * lane]) * gam;
    yv[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[h] = -1e30f;
    l[h] = 0.f;
  }
  f32x4 od = {0.f, 0.f, 0.f, 0.f};
  // the next shared row is loaded while this one is worked on
  f32x4 xn = {0.f, 0.f, 0.f, 0.f};
  float rn = 0.f;
  if (hw < p.I && !(hw >= p.ded0 && hw < p.ded1)) {
    xn = ld4(p.x + (row0 + hw) * p.ldx + 4 * lane);
    rn = p.rstd[row0 + hw];
  }
  for (int j = hw; j < p.I; j += NHW) {
    const int64_t r = row0 + j;
    const f32x4 xc = xn;
    const float rc = rn;
    const int jn = j + NHW;
    if (jn < p.I && !(jn >= p.ded0 && jn < p.ded1)) {
      xn = ld4(p.x + (row0 + jn) * p.ldx + 4 * lane);
      rn = p.rstd[row0 + jn];
    }
    if (j >= p.ded0 && j < p.ded1) {              // dedicated key: its projected K / V rows
      const f32x4 kv = ld4(p.qkv + r * p.ldqkv + FD + 4 * lane);
      const f32x4 vv = ld4(p.qkv + r * p.ldqkv + 2 * FD + 4 * lane);
      const float dt = dot4(kv, q4);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float s = half_sum(myh == h ? dt : 0.f) * p.scale;
        const float mn = fmaxf(m[h], s);
        const float corr = __expf(m[h] - mn), pe = __expf(s - mn);
        l[h] = l[h] * corr + pe;
        m[h] = mn;
        yv[h] = yv[h] * corr;
        if (myh == h) od = od * corr + vv * pe;
      }
    } else {                                      // shared key: the raw row against the folded query
      const f32x4 xv = xc * rc;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float s = half_sum(dot4(xv, qth[h])) * p.scale;
        const float mn = fmaxf(m[h], s);
        const float corr = __expf(m[h] - mn), pe = __expf(s - mn);
        l[h] = l[h] * corr + pe;
        m[h] = mn;
        yv[h] = yv[h] * corr + xv * pe;
        if (myh == h) od = od * corr;
      }
    }
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    st4(&ry[hw][h][4 * lane], yv[h]);
    if (lane == 0) { rm[hw][h] = m[h]; rl[hw][h] = l[h]; }
  }
  st4(&ro[hw][4 * lane], od);
  __syncthreads();
  // merge the eight states in half-wave order
  for (int idx = t; idx < H * FD; idx += 256) {
    const int h = idx / FD, k = idx % FD;
    float M = rm[0][h];
#pragma unroll
    for (int w = 1; w < NHW; ++w) M = fmaxf(M, rm[w][h]);
    float L = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < NHW; ++w) {
      const float e = __expf(rm[w][h] - M);
      L += rl[w][h] * e;
      a += ry[w][h][k] * e;
    }
    a /= L;
    p.y[((int64_t)b * H + h) * FD + k] = a;
    gy[h][k] = a * p.gamma[k];
    if (k == 0) p.lse[(int64_t)b * H + h] = M + __logf(L);
  }
  __syncthreads();
  head_matvec<H>(p.w, p.ldw, 2 * FD, gy, po, t);
  __syncthreads();
  if (t < FD) {
    const int h = t / HD;
    float M = rm[0][h];
#pragma unroll
    for (int w = 1; w < NHW; ++w) M = fmaxf(M, rm[w][h]);
    float L = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < NHW; ++w) {
      const float e = __expf(rm[w][h] - M);
      L += rl[w][h] * e;
      a += ro[w][t] * e;
    }
    p.o[(int64_t)b * FD + t] = (po[0][t] + po[1][t]) + a / L;
  }
}

template <int H>
__global__ __launch_bounds__(256) void attn_fold_bwd_kernel(FoldArgs p) {
  constexpr int HD = FD / H, LPH = 32 / H;
  __shared__ __attribute__((aligned(16))) float qs[FD];
  __shared__ __attribute__((aligned(16))) float dos[FD];
  __shared__ __attribute__((aligned(16))) float ab[2][H][FD];    // a_h = Wk0[:, h] q_h, b_h = Wv0[:, h] do_h
  __shared__ __attribute__((aligned(16))) float rz[NHW][H][FD];
  __shared__ __attribute__((aligned(16))) float rq[NHW][FD];
  __shared__ float gz[H][FD];
  __shared__ float po[2][FD];
  const int b = blockIdx.x, t = threadIdx.x, hw = t >> 5, lane = t & 31, myh = lane / LPH;
  const int64_t row0 = (int64_t)b * p.I;
  if (t < FD) {
    qs[t] = p.qkv[(row0 + p.I - 1) * p.ldqkv + t];
    dos[t] = p.dout[(int64_t)b * FD + t];
  }
  __syncthreads();
  head_matvec_T<H>(p.wT, p.ldwT, FD, qs, ab[0], t);
  head_matvec_T<H>(p.wT, p.ldwT, 2 * FD, dos, ab[1], t);
  __syncthreads();
  const f32x4 gam = ld4(p.gamma + 4 * lane);
  const f32x4 q4 = ld4(qs + 4 * lane), do4 = ld4(dos + 4 * lane);
  f32x4 qth[H], ch[H], zv[H];
  float lse[H], delta[H];
  const float od = dot4(ld4(p.o + (int64_t)b * FD + 4 * lane), do4);
#pragma unroll
  for (int h = 0; h < H; ++h) {
    qth[h] = ld4(&ab[0][h][4 * lane]) * gam;
    ch[h] = ld4(&ab[1][h][4 * lane]) * gam;
    zv[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    lse[h] = p.lse[(int64_t)b * H + h];
    delta[h] = half_sum(myh == h ? od : 0.f);
  }
  f32x4 dqd = {0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bool q_ded = p.I - 1 >= p.ded0 && p.I - 1 < p.ded1;      // is the query row a dedicated key?
  f32x4 xn = zero4;                                               // the next shared row, loaded one pass ahead
  float rn = 0.f;
  if (hw < p.I && !(hw >= p.ded0 && hw < p.ded1)) {
    xn = ld4(p.x + (row0 + hw) * p.ldx + 4 * lane);
    rn = p.rstd[row0 + hw];
  }
  for (int j = hw; j < p.I; j += NHW) {
    const int64_t r = row0 + j;
    const bool isq = j == p.I - 1;
    const f32x4 xc = xn;
    const float rc = rn;
    const int jn = j + NHW;
    if (jn < p.I && !(jn >= p.ded0 && jn < p.ded1)) {
      xn = ld4(p.x + (row0 + jn) * p.ldx + 4 * lane);
      rn = p.rstd[row0 + jn];
    }
    const f32x4 res = (isq && p.dx1) ? ld4(p.dx1 + (int64_t)b * FD + 4 * lane) : zero4;   // the query row's residual
    if (j >= p.ded0 && j < p.ded1) {
      const f32x4 kv = ld4(p.qkv + r * p.ldqkv + FD + 4 * lane);
      const f32x4 vv = ld4(p.qkv + r * p.ldqkv + 2 * FD + 4 * lane);
      const float dt = dot4(kv, q4), dtv = dot4(vv, do4);
      float dsm = 0.f, pm = 0.f;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float s = half_sum(myh == h ? dt : 0.f) * p.scale;
        const float pr = __expf(s - lse[h]);
        const float dp = half_sum(myh == h ? dtv : 0.f);
        const float ds = pr * (dp - delta[h]) * p.scale;
        if (myh == h) { dsm = ds; pm = pr; }
      }
      dqd = dqd + kv * dsm;
      float* crow = p.dqkv + ((int64_t)b * p.nf + (j - p.ded0)) * p.lddqkv + 4 * lane;
      if (!isq) st4(crow, zero4);                                 // (the query row's dq is written at the end)
      st4(crow + FD, q4 * dsm);
      st4(crow + 2 * FD, do4 * pm);
      st4(p.dx + r * p.lddx + 4 * lane, res);                     // the map-row dgrad adds onto it
    } else {
      const float rs = rc;
      const f32x4 xv = xc * rs;
      f32x4 g = zero4;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float s = half_sum(dot4(xv, qth[h])) * p.scale;
        const float pr = __expf(s - lse[h]);
        const float dp = half_sum(dot4(xv, ch[h]));
        const float ds = pr * (dp - delta[h]) * p.scale;
        zv[h] = zv[h] + xv * ds;
        g = g + qth[h] * ds + ch[h] * pr;
      }
      const float gx = half_sum(dot4(g, xv)) * (1.f / FD);
      st4(p.dx + r * p.lddx + 4 * lane, (g - xv * gx) * rs + res);
    }
  }
#pragma unroll
  for (int h = 0; h < H; ++h) st4(&rz[hw][h][4 * lane], zv[h]);
  st4(&rq[hw][4 * lane], dqd);
  __syncthreads();
  for (int idx = t; idx < H * FD; idx += 256) {
    const int h = idx / FD, k = idx % FD;
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NHW; ++w) a += rz[w][h][k];
    p.z[((int64_t)b * H + h) * FD + k] = a;
    gz[h][k] = a * p.gamma[k];
    rz[0][h][k] = a;                               // (this thread alone reads and writes column (h, k))
  }
  __syncthreads();
  head_matvec<H>(p.w, p.ldw, FD, gz, po, t);
  if (t < FD) {                                    // this sample's part of dgamma
    float a = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h)
      a += rz[0][h][t] * ab[0][h][t] + p.y[((int64_t)b * H + h) * FD + t] * ab[1][h][t];
    p.dgpart[(int64_t)b * FD + t] = a;
  }
  __syncthreads();
  if (t < FD) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NHW; ++w) a += rq[w][t];
    float* crow = p.dqkv + ((int64_t)b * p.nf + (q_ded ? p.I - 1 - p.ded0 : p.ded1 - p.ded0)) * p.lddqkv;
    crow[t] = (po[0][t] + po[1][t]) + a;
    if (!q_ded) { crow[FD + t] = 0.f; crow[2 * FD + t] = 0.f; }
  }
}

// part[chunk][kv][k][n] = sum over the chunk's samples of A[b][head(n)][k] D[b][n]; kv 0: A = z, D = q; kv 1: A = y,
// D = do.  Thread (k = t & 127, half = t >> 7) holds columns 64 half .. 64 half + 63.
template <int H>
__global__ __launch_bounds__(256) void attn_fold_dw_kernel(const float* z, const float* y, const float* qkv,
                                                           int64_t ldqkv, const float* dout, int B, int I,
                                                           float* part) {
  constexpr int HD = FD / H, HPH = 64 / HD;       // heads per column half
  __shared__ __attribute__((aligned(16))) float dsm[DW_ROWS][FD];
  const int t = threadIdx.x, kv = blockIdx.y, b0 = blockIdx.x * DW_ROWS;
  const int nb = min(DW_ROWS, B - b0);
  const float* A = kv ? y : z;
  for (int idx = t; idx < nb * FD; idx += 256) {
    const int64_t bb = b0 + idx / FD;
    const int n = idx % FD;
    dsm[idx / FD][n] = kv ? dout[bb * FD + n] : qkv[(bb * I + I - 1) * ldqkv + n];
  }
  __syncthreads();
  const int k = t & (FD - 1), half = t >> 7;
  float acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = 0.f;
#pragma unroll 2
  for (int bb = 0; bb < nb; ++bb) {
#pragma unroll
    for (int hh = 0; hh < HPH; ++hh) {
      const int h = half * HPH + hh;
      const float a = A[((int64_t)(b0 + bb) * H + h) * FD + k];
#pragma unroll
      for (int c = 0; c < HD; c += 4) {
        const f32x4 dv = ld4(&dsm[bb][h * HD + c]);
        acc[hh * HD + c + 0] = fmaf(a, dv.x, acc[hh * HD + c + 0]);
        acc[hh * HD + c + 1] = fmaf(a, dv.y, acc[hh * HD + c + 1]);
        acc[hh * HD + c + 2] = fmaf(a, dv.z, acc[hh * HD + c + 2]);
        acc[hh * HD + c + 3] = fmaf(a, dv.w, acc[hh * HD + c + 3]);
      }
    }
  }
  float* out = part + (((int64_t)blockIdx.x * 2 + kv) * FD + k) * FD + half * 64;
#pragma unroll
  for (int c = 0; c < 64; c += 4) st4(out + c, f32x4{acc[c], acc[c + 1], acc[c + 2], acc[c + 3]});
}

// dW[k][d + kv d + n] (+)= gamma[k] sum_chunk part[chunk][kv][k][n], chunks in order
__global__ __launch_bounds__(256) void attn_fold_dw_reduce_kernel(const float* part, int nchunk, const float* gamma,
                                                                  float* dW, int64_t lddw, int accumulate) {
  const int idx = blockIdx.x * 256 + threadIdx.x;           // < 2 FD FD
  const int kv = idx / (FD * FD), k = (idx / FD) % FD, n = idx % FD;
  float a = 0.f;
#pragma unroll 8
  for (int c = 0; c < nchunk; ++c) a += part[((int64_t)c * 2 + kv) * FD * FD + k * FD + n];
  a *= gamma[k];
  float* dst = dW + (int64_t)k * lddw + FD + kv * FD + n;
  *dst = accumulate ? *dst + a : a;
}

// environment variable ONETRANS_LAST_FOLD (0 / 1) sets the process's initial value
static int last_fold_initial() {
  const char* e = getenv("ONETRANS_LAST_FOLD");
  return e && *e ? (atoi(e) != 0) : 1;
}
static std::atomic<int> g_last_fold{last_fold_initial()};

static bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int check_common(const char* fn, const float* x, int64_t ldx, const float* rstd, const float* gamma,
                        const float* w, int64_t ldw, const float* wT, int64_t ldwT, const float* qkv, int64_t ldqkv,
                        int B, int H, int I, int head_dim, int ded0, int ded1) {
  OT_REQUIRE(x && rstd && gamma && w && wT && qkv, "%s: null operand", fn);
  OT_REQUIRE(B >= 0 && I >= 1 && (int64_t)B * I < (int64_t)1 << 31, "%s: bad B / I", fn);
  if (!ot_attn_fold_supported(H * head_dim, H))
    return fail(OT_ERR_UNSUPPORTED, "%s: width %d with %d heads is not built (128 with 2 or 4 heads)", fn,
                H * head_dim, H);
  OT_REQUIRE(0 <= ded0 && ded0 <= ded1 && ded1 <= I, "%s: dedicated range [%d, %d) outside [0, %d]", fn, ded0, ded1,
             I);
  OT_REQUIRE(ldx >= FD && ldx % 4 == 0 && ldqkv >= 3 * FD && ldqkv % 4 == 0 && ldw >= 3 * FD && ldwT >= FD,
             "%s: leading dimensions", fn);
  OT_REQUIRE(a16(x) && a16(gamma) && a16(qkv), "%s: x, gamma and qkv must be 16-byte aligned", fn);
  return OT_OK;
}

}  // namespace fold
}  // namespace ot

using namespace ot;
using namespace ot::fold;

extern "C" int ot_last_fold(int on) {
  const int old = g_last_fold.load(std::memory_order_relaxed);
  if (on >= 0) g_last_fold.store(on ? 1 : 0, std::memory_order_relaxed);
  return old;
}

extern "C" int ot_attn_fold_supported(int d, int H) { return d == FD && (H == 2 || H == 4); }

extern "C" int ot_attn_fold_fwd(const float* x, int64_t ldx, const float* rstd, const float* gamma, const float* w,
                                int64_t ldw, const float* wT, int64_t ldwT, const float* qkv, int64_t ldqkv, int B,
                                int H, int I, int head_dim, int ded0, int ded1, float* o, float* lse, float* y,
                                void* stream) {
  OT_TRY(check_common("ot_attn_fold_fwd", x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, head_dim, ded0,
                      ded1));
  OT_REQUIRE(o && lse && y, "ot_attn_fold_fwd: null output");
  if (B == 0) return OT_OK;
  FoldArgs p{};
  p.x = x; p.ldx = ldx; p.rstd = rstd; p.gamma = gamma; p.w = w; p.ldw = ldw; p.wT = wT; p.ldwT = ldwT;
  p.qkv = qkv; p.ldqkv = ldqkv; p.B = B; p.I = I; p.ded0 = ded0; p.ded1 = ded1;
  p.scale = 1.0f / sqrtf((float)head_dim);
  p.o = o; p.lse = lse; p.y = y;
  if (H == 2) hipLaunchKernelGGL(attn_fold_fwd_kernel<2>, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(attn_fold_fwd_kernel<4>, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  OT_LAUNCH_CHECK("ot_attn_fold_fwd");
  return OT_OK;
}

extern "C" int ot_attn_fold_bwd(const float* x, int64_t ldx, const float* rstd, const float* gamma, const float* w,
                                int64_t ldw, const float* wT, int64_t ldwT, const float* qkv, int64_t ldqkv, int B,
                                int H, int I, int head_dim, int ded0, int ded1, const float* o, const float* dout,
                                const float* lse, const float* y, const float* dx1, float* dx, int64_t lddx,
                                float* dqkv, int64_t lddqkv, float* z, float* dgpart, void* stream) {
  OT_TRY(check_common("ot_attn_fold_bwd", x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, head_dim, ded0,
                      ded1));
  OT_REQUIRE(o && dout && lse && y && dx && dqkv && z && dgpart, "ot_attn_fold_bwd: null operand");
  OT_REQUIRE(lddx >= FD && lddx % 4 == 0 && lddqkv >= 3 * FD && lddqkv % 4 == 0, "ot_attn_fold_bwd: leading dimensions");
  OT_REQUIRE(a16(o) && a16(dx) && a16(dqkv) && (!dx1 || a16(dx1)),
             "ot_attn_fold_bwd: o, dx, dqkv and dx1 must be 16-byte aligned");
  if (B == 0) return OT_OK;
  FoldArgs p{};
  p.x = x; p.ldx = ldx; p.rstd = rstd; p.gamma = gamma; p.w = w; p.ldw = ldw; p.wT = wT; p.ldwT = ldwT;
  p.qkv = qkv; p.ldqkv = ldqkv; p.B = B; p.I = I; p.ded0 = ded0; p.ded1 = ded1;
  p.scale = 1.0f / sqrtf((float)head_dim);
  p.o = const_cast<float*>(o); p.lse = const_cast<float*>(lse); p.y = const_cast<float*>(y);
  p.dout = dout; p.dx1 = dx1; p.dx = dx; p.lddx = lddx; p.dqkv = dqkv; p.lddqkv = lddqkv;
  p.nf = ot_attn_fold_rows(I, ded0, ded1);
  p.z = z; p.dgpart = dgpart;
  if (H == 2) hipLaunchKernelGGL(attn_fold_bwd_kernel<2>, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(attn_fold_bwd_kernel<4>, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  OT_LAUNCH_CHECK("ot_attn_fold_bwd");
  return OT_OK;
}

extern "C" int ot_attn_fold_rows(int I, int ded0, int ded1) {
  return (ded1 - ded0) + ((I - 1 >= ded0 && I - 1 < ded1) ? 0 : 1);
}

extern "C" size_t ot_attn_fold_workspace_size(int B, int d) {
  const int64_t nchunk = ceil_div(B, DW_ROWS);
  const int64_t dw = nchunk * 2 * d * d, dg = colsum_scratch_floats(B, d);
  return (size_t)(dw > dg ? dw : dg) * sizeof(float);
}

extern "C" int ot_attn_fold_dw(const float* z, const float* y, const float* qkv, int64_t ldqkv, const float* dout,
                               const float* gamma, int B, int H, int I, int head_dim, float* dW, int64_t lddw,
                               int accumulate, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(z && y && qkv && dout && gamma && dW, "ot_attn_fold_dw: null operand");
  if (!ot_attn_fold_supported(H * head_dim, H))
    return fail(OT_ERR_UNSUPPORTED, "ot_attn_fold_dw: width %d with %d heads is not built", H * head_dim, H);
  OT_REQUIRE(B >= 0 && I >= 1 && ldqkv >= 3 * FD && lddw >= 3 * FD, "ot_attn_fold_dw: bad sizes");
  OT_REQUIRE(workspace && ws_bytes >= ot_attn_fold_workspace_size(B, FD) && a16(workspace),
             "ot_attn_fold_dw: workspace too small");
  const unsigned nchunk = ceil_div(B, DW_ROWS);
  float* part = (float*)workspace;
  if (nchunk > 0) {
    if (H == 2)
      hipLaunchKernelGGL(attn_fold_dw_kernel<2>, dim3(nchunk, 2), dim3(256), 0, (hipStream_t)stream, z, y, qkv, ldqkv,
                         dout, B, I, part);
    else
      hipLaunchKernelGGL(attn_fold_dw_kernel<4>, dim3(nchunk, 2), dim3(256), 0, (hipStream_t)stream, z, y, qkv, ldqkv,
                         dout, B, I, part);
    OT_LAUNCH_CHECK("ot_attn_fold_dw");
  }
  hipLaunchKernelGGL(attn_fold_dw_reduce_kernel, dim3(2 * FD * FD / 256), dim3(256), 0, (hipStream_t)stream, part,
                     (int)nchunk, gamma, dW, lddw, accumulate);
  OT_LAUNCH_CHECK("ot_attn_fold_dw(reduce)");
  return OT_OK;
}

extern "C" int ot_attn_fold_dgamma(const float* dgpart, int B, int d, float* dgamma, int accumulate, void* workspace,
                                   size_t ws_bytes, void* stream) {
  OT_REQUIRE(dgpart && dgamma && B >= 0 && d > 0, "ot_attn_fold_dgamma: bad args");
  OT_REQUIRE(workspace && ws_bytes >= ot_attn_fold_workspace_size(B, d), "ot_attn_fold_dgamma: workspace too small");
  launch_colsum_reduce(dgpart, B, d, dgamma, accumulate, (hipStream_t)stream, (float*)workspace);
  OT_LAUNCH_CHECK("ot_attn_fold_dgamma");
  return OT_OK;
}
