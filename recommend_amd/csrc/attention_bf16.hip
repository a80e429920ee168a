// Causal attention with a query tail on bf16 MFMA (v_mfma_f32_32x32x16_bf16), operands as bf16 planes: the
// split-plane forward (attn_fwd_split_kernel), the one-plane backward per (sample, head) wave
// (attn_bwd_split_kernel) and the key-grouped backward for long tails (attn_bwd_group_kernel with
// attn_dq_reduce_kernel).  attention.hip routes a call here; attn.h has the layout.
#include <mutex>

#include "attn.h"

namespace ot {

// XOR-swizzled byte offset in a bf16 image of RB-byte rows (the split forward's V planes, the key-grouped
// backward's [32][HD] and [32][32] images): row r's 16-B chunk index is XORed with (r / (256 / RB)) mod (RB / 16),
// so the rows that share LDS banks (256 B apart) spread over the chunks — the row-major fragment reads (one row per
// lane) and the transposed reads were 2- to 8-way bank-conflicted on the plain layout (C5: conflict cycles 68% of
// the LDS-active cycles; the plain layout was a compile-time switch until it was retired).
template <int RB>
__device__ __forceinline__ int gswz(int r, int b) {
  constexpr int P = 256 / RB, C = RB / 16;
  return r * RB + (b ^ (((r / P) & (C - 1)) << 4));
}
template <int RB>
__device__ __forceinline__ u32x4 tr16_frag_sw(const char* img, int ra, int rb, int colbase, int lane) {
  typedef short v4i16 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
  const int gi = lane & 15, q = gi >> 2, pp = gi & 3;
  const int c = colbase + 16 * ((lane >> 4) & 1) + 4 * pp;
  const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + gswz<RB>(ra + q, c * 2)));
  const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + gswz<RB>(rb + q, c * 2)));
  const u32x2 a = __builtin_bit_cast(u32x2, lo), b = __builtin_bit_cast(u32x2, hi);
  return u32x4{a.x, a.y, b.x, b.y};
}

// Split-bf16 forward (OT_MATMUL_SPLIT_BF16; HD >= 32): the same online softmax as attn_fwd_kernel,
// the two products on v_mfma_f32_32x32x16_bf16 with every f32 operand split exactly into three bf16
// planes and the six largest plane products summed (mfma_split6: f32-accurate, 2.7x fewer MFMA
// cycles than the 32x32x2 f32 form).
//   S^T = K Q^T: K (A, lane = key) and Q (B, lane = query) fragments split in registers; lane half
//     hh, k-step t, element j <-> dim (HD/2) hh + 8t + j on both sides.
//   O^T += V^T P^T: P^T is the S^T accumulator (k-step s = registers 8s..8s+7, element j <-> key
//     16s + 8(j>>2) + 4hh + (j&3)); V^T comes from the wave's row-major bf16 V plane images through
//     ds_read_b64_tr_b16 (4 key rows of the lane's dim column per read, two reads per k-step).
template <int HD>
__device__ __forceinline__ u32x4 vt_frag(const char* plane, int s, int c, int lane) {
  // lane 4q+p of each 16-lane group addresses key row r0 + q, dims c0 + 4p .. c0 + 4p + 3
  typedef short v4i16 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
  const int hh = lane >> 5, gi = lane & 15, q = gi >> 2, pp = gi & 3;
  const int c0 = 32 * c + 16 * ((lane >> 4) & 1) + 4 * pp;
  const int r0 = 16 * s + 4 * hh + q;
  const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(plane + gswz<HD * 2>(r0, c0 * 2)));
  const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(plane + gswz<HD * 2>(r0 + 8, c0 * 2)));
  const u32x2 a = __builtin_bit_cast(u32x2, lo), b = __builtin_bit_cast(u32x2, hi);
  return u32x4{a.x, a.y, b.x, b.y};
}

template <int HD, int TERMS>
__global__ __launch_bounds__(256) void attn_fwd_split_kernel(AttnArgs p) {
  static_assert(HD >= 32, "split forward: HD >= 32");
  constexpr int NS = HD / 16;                         // k-steps of S^T
  constexpr int PLANE = 32 * HD * 2;                  // bytes of one V plane image [32 keys][HD] bf16
  __shared__ __attribute__((aligned(16))) char lds[4][3 * PLANE];
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  char* vimg = lds[threadIdx.x >> 6];
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= p.B * p.H) return;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K;
  const float* Q = p.qkv + (int64_t)b * I * p.ld + h * HD;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  const int32_t* qp = p.qpos ? p.qpos + (int64_t)b * K : nullptr;
  const int nqb = (K + 31) / 32;
  const float qscale = p.scale * 1.4426950408889634f;   // log2(e) / sqrt(hd)
  for (int qb = 0; qb < nqb; ++qb) {
    const int j = 32 * qb + li;
    const int qpos = query_pos(qp, q_off, j < K ? j : K - 1);
    u32x4 qs[NS][3];
    {
      float qf[HD / 2];
      load_frag_clamped<HD>(qf, Q, p.ld, qpos, I, hh);
#pragma unroll
      for (int s = 0; s < HD / 2; ++s) qf[s] *= qscale;
#pragma unroll
      for (int t = 0; t < NS; ++t) split8t<TERMS>(qf + 8 * t, qs[t]);
    }
    f32x16 oacc[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int last_q = query_pos(qp, q_off, min(32 * qb + 31, K - 1));
    const int nkb = last_q / 32 + 1;
    const int first_masked = query_pos(qp, q_off, 32 * qb) / 32;
    // K/V fragments of key block kb + 1 are loaded while block kb computes (the global latency
    // would otherwise be exposed once per block)
    float kf[HD / 2], vf[HD / 2];
    load_frag<HD>(kf, Kp, p.ld, li, I, hh);
    load_frag<HD>(vf, V, p.ld, li, I, hh);
    for (int kb = 0; kb < nkb; ++kb) {
      const int key0 = 32 * kb;
      float kn[HD / 2], vn[HD / 2];
      load_frag<HD>(kn, Kp, p.ld, kb + 1 < nkb ? key0 + 32 + li : I, I, hh);    // rows >= I: no load
      load_frag<HD>(vn, V, p.ld, kb + 1 < nkb ? key0 + 32 + li : I, I, hh);
      f32x16 sacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
      {
        // V planes -> the wave's row-major images (row = key li, dims (HD/2) hh ..)
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          u32x4 vp[3];
          split8t<TERMS>(vf + 8 * t, vp);
#pragma unroll
          for (int pl = 0; pl < (TERMS == 1 ? 1 : 3); ++pl)
            *reinterpret_cast<u32x4*>(vimg + pl * PLANE + gswz<HD * 2>(li, ((HD / 2) * hh + 8 * t) * 2)) = vp[pl];
        }
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          u32x4 ks[3];
          split8t<TERMS>(kf + 8 * t, ks);
          sacc = mfma_terms<TERMS>(ks, qs[t], sacc);         // S^T (log2 units): row = key, col = query
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < HD / 2; ++s2) { kf[s2] = kn[s2]; vf[s2] = vn[s2]; }
      f32x16 s = sacc;
      if (kb >= first_masked) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          s[r] = (key0 + acc_row(r, hh) <= qpos) ? s[r] : -INFINITY;
      }
      float mloc = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, s[r]);
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
      const float mnew = fmaxf(m, mloc);
      const float corr = __builtin_amdgcn_exp2f(m - mnew);
      float lsum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[r] - mnew);
        s[r] = e;
        lsum += e;
      }
      lsum += __shfl_xor(lsum, 32, 64);
      l = l * corr + lsum;
      m = mnew;
#pragma unroll
      for (int c = 0; c < NB(HD); ++c) oacc[c] *= corr;
      u32x4 ps[2][3];
      {
        float pv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) pv[r] = s[r];
        split8t<TERMS>(pv, ps[0]);
        split8t<TERMS>(pv + 8, ps[1]);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4 va[3];
#pragma unroll
          for (int pl = 0; pl < (TERMS == 1 ? 1 : 3); ++pl) va[pl] = vt_frag<HD>(vimg + pl * PLANE, st, c, lane);
          oacc[c] = mfma_terms<TERMS>(va, ps[st], oacc[c]);   // O^T += V^T P^T
        }
      __builtin_amdgcn_wave_barrier();
    }
    if (j < K) {
      const float inv = 1.f / l;
      float* orow = p.out + ((int64_t)b * K + j) * p.d + h * HD;
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = 32 * c + 8 * g + 4 * hh;
          f32x4 v = {oacc[c][4 * g] * inv, oacc[c][4 * g + 1] * inv, oacc[c][4 * g + 2] * inv,
                     oacc[c][4 * g + 3] * inv};
          *reinterpret_cast<f32x4*>(orow + dd) = v;
        }
      if (hh == 0) p.lse[((int64_t)b * p.H + h) * K + j] = m * 0.6931471805599453f + __logf(l);
    }
  }
}

// ------------------------------------------------------------------------------------------
// bf16 backward (TERMS = 1, OT_MATMUL_BF16; the kernel also builds with TERMS = 6 split planes, which
// measured slower than attn_bwd_kernel and is not dispatched).
// Same pass structure as attn_bwd_kernel (one wave per (sample, head), key blocks outer, the query
// blocks that see them inner, dQ partial read-modify-written in dqkv), all five products on
// v_mfma_f32_32x32x16_bf16:
//   S = Q K^T, dP = dO V^T        A = Q / dO (lane = query), B = K / V (lane = key): register planes
//   dV^T += dO^T P, dK^T += Q^T dS  A = dO^T / Q^T via ds_read_b64_tr_b16 from the wave's row-major
//                                  [query][dim] plane images (k = query in the accumulator order of
//                                  P / dS, which are the B operands straight from the registers)
//   dQ^T += K^T dS^T              A = K^T from the [key][dim] image, B = dS^T from a [key][query]
//                                  image the lanes write as 8-byte runs (k = key, natural order)
// K and V fragments (the B operands of S and dP) are re-read from the wave's [key][dim] plane images
// each pair instead of living in registers for the whole key block: at HD 64 the kernel fits 256
// registers, i.e. 2 waves / SIMD instead of 1 (C5 backward 17.4 -> see DESIGN.md).
// Planes: 3 (split, TERMS = 6) or 1 (bf16).  LDS per wave: (4 x 32 x HD + 32 x 32) x 2 B x planes.

// two ds_read_b64_tr_b16 reads -> one 32x32x16 operand fragment: elements 0-3 from rows ra .. ra+3,
// 4-7 from rows rb .. rb+3, the lane's column colbase + (lane & 31) (row stride rs bytes)
__device__ __forceinline__ u32x4 tr16_frag(const char* img, int rs, int ra, int rb, int colbase, int lane) {
  typedef short v4i16 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
  const int gi = lane & 15, q = gi >> 2, pp = gi & 3;
  const int c = colbase + 16 * ((lane >> 4) & 1) + 4 * pp;
  const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + (ra + q) * rs + c * 2));
  const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + (rb + q) * rs + c * 2));
  const u32x2 a = __builtin_bit_cast(u32x2, lo), b = __builtin_bit_cast(u32x2, hi);
  return u32x4{a.x, a.y, b.x, b.y};
}

template <int HD, int TERMS>
constexpr int BWDS_LDS() { return (TERMS == 1 ? 1 : 3) * (4 * 32 * HD + 32 * 32) * 2; }

template <int HD, int TERMS, bool SEL, int WAVES>
__global__ __launch_bounds__(64 * WAVES, TERMS == 1 ? 2 : 1) void attn_bwd_split_kernel(AttnArgs p) {
  static_assert(HD == 32 || HD == 64, "split backward: HD 32 or 64");
  constexpr int NPL = TERMS == 1 ? 1 : 3;
  constexpr int NS = HD / 16;                          // k-steps over the head dim
  constexpr int IMG = 32 * HD * 2;                     // bytes of one [32][HD] plane image
  constexpr int SIMG = 32 * 32 * 2;                    // bytes of one [32 keys][32 queries] plane
  extern __shared__ __attribute__((aligned(16))) char lds_b[];
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  char* kimg = lds_b + (threadIdx.x >> 6) * BWDS_LDS<HD, TERMS>();
  char* qimg = kimg + NPL * IMG;
  char* oimg = qimg + NPL * IMG;
  char* simg = oimg + NPL * IMG;
  char* vimg = simg + NPL * SIMG;
  const int pair = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (pair >= p.B * p.H) return;                       // wave-uniform
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K, KP = attn_kpad(K);
  const int64_t tok0 = (int64_t)b * I;
  const float* Q = p.qkv + tok0 * p.ld + h * HD;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  const float* dO = p.dout + (int64_t)b * K * p.d + h * HD;
  const float* lsep = p.delta + (int64_t)pair * KP;
  const float* dltp = p.delta + ((int64_t)p.B * p.H + pair) * KP;
  const int32_t* qpp = reinterpret_cast<const int32_t*>(p.delta + 2 * (int64_t)p.B * p.H * KP) + (int64_t)b * KP;
  float* dK = p.dqkv + tok0 * p.ld + p.d + h * HD;
  float* dV = dK + p.d;
  const int nqb = KP / 32;
  const int nkb = (I + 31) / 32;
  auto qrow = [&](int j) { return SEL ? qpp[j < KP ? j : KP - 1] : q_off + (j < K ? j : K - 1); };

  for (int kb = 0; kb < nkb; ++kb) {
    const int key0 = 32 * kb;
    const int kpos = key0 + li;
    {
      float kf[HD / 2], vf[HD / 2];
      load_frag<HD>(kf, Kp, p.ld, kpos, I, hh);        // rows >= I: zeros (masked below)
      load_frag<HD>(vf, V, p.ld, kpos, I, hh);
#pragma unroll
      for (int t = 0; t < NS; ++t) {
        u32x4 kB[3], vB[3];
        split8t<TERMS>(kf + 8 * t, kB);
        split8t<TERMS>(vf + 8 * t, vB);
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          *reinterpret_cast<u32x4*>(kimg + pl * IMG + (li * HD + (HD / 2) * hh + 8 * t) * 2) = kB[pl];
          *reinterpret_cast<u32x4*>(vimg + pl * IMG + (li * HD + (HD / 2) * hh + 8 * t) * 2) = vB[pl];
        }
      }
    }
    f32x16 dk[NB(HD)], dv[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) { dk[c][r] = 0.f; dv[c][r] = 0.f; }
    int qb0;
    if constexpr (SEL) {
      qb0 = 0;
      while (qb0 < nqb - 1 && qpp[32 * qb0 + 31] < key0) ++qb0;
    } else {
      qb0 = key0 - q_off; qb0 = qb0 < 0 ? 0 : qb0 / 32;
    }
    for (int qb = qb0; qb < nqb; ++qb) {
      const int q0 = 32 * qb;
      const int jq = q0 + li;
      // Q / dO rows of this lane's query: register planes (A of S / dP) and the plane images
      u32x4 qA[NS][3], oA[NS][3];
      {
        float qf[HD / 2], of[HD / 2];
        if constexpr (SEL) load_frag<HD>(qf, Q, p.ld, jq < K ? qpp[jq] : I, I, hh);
        else load_frag<HD>(qf, Q, p.ld, jq < K ? q_off + jq : I, I, hh);
        load_frag<HD>(of, dO, p.d, jq, K, hh);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          split8t<TERMS>(qf + 8 * t, qA[t]);
          split8t<TERMS>(of + 8 * t, oA[t]);
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
            *reinterpret_cast<u32x4*>(qimg + pl * IMG + (li * HD + (HD / 2) * hh + 8 * t) * 2) = qA[t][pl];
            *reinterpret_cast<u32x4*>(oimg + pl * IMG + (li * HD + (HD / 2) * hh + 8 * t) * 2) = oA[t][pl];
          }
        }
      }
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int t = 0; t < NS; ++t) {
        u32x4 kB[3], vB[3];                              // this lane's key row, dims 8t.. (its own writes)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          kB[pl] = *reinterpret_cast<const u32x4*>(kimg + pl * IMG + (li * HD + (HD / 2) * hh + 8 * t) * 2);
          vB[pl] = *reinterpret_cast<const u32x4*>(vimg + pl * IMG + (li * HD + (HD / 2) * hh + 8 * t) * 2);
        }
        s = mfma_terms<TERMS>(qA[t], kB, s);            // S: row = query, col = key
        dp = mfma_terms<TERMS>(oA[t], vB, dp);          // dP
      }
      // softmax gradient (rows = queries acc_row(r, hh), column = this lane's key)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(lsep + q0 + 8 * g + 4 * hh);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(dltp + q0 + 8 * g + 4 * hh);
        i32x4 qv4;
        if constexpr (SEL) qv4 = *reinterpret_cast<const i32x4*>(qpp + q0 + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e, j = q0 + 8 * g + 4 * hh + e;
          const int qposj = SEL ? qv4[e] : q_off + j;
          const float ex = __expf(s[r] * p.scale - l4[e]);
          const float P = kpos <= qposj ? ex : 0.f;
          s[r] = P;
          dp[r] = P * (dp[r] - d4[e]) * p.scale;         // dS, pre-scaled by 1/sqrt(hd)
        }
      }
      u32x4 pB[2][3], sB[2][3];
      {
        float pv[16], sv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { pv[r] = s[r]; sv[r] = dp[r]; }
        split8t<TERMS>(pv, pB[0]); split8t<TERMS>(pv + 8, pB[1]);
        split8t<TERMS>(sv, sB[0]); split8t<TERMS>(sv + 8, sB[1]);
        // dS^T image [key][query]: this lane's key row, registers 4g .. 4g+3 = queries 8g + 4hh + 0..3
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const u32x4 w = sB[g >> 1][pl];
            const u32x2 two = (g & 1) ? u32x2{w.z, w.w} : u32x2{w.x, w.y};
            *reinterpret_cast<u32x2*>(simg + pl * SIMG + (li * 32 + 8 * g + 4 * hh) * 2) = two;
          }
      }
      __builtin_amdgcn_wave_barrier();
      // dV^T += dO^T P, dK^T += Q^T dS  (k = query, accumulator order)
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4 oT[3], qT[3];
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
            oT[pl] = tr16_frag(oimg + pl * IMG, HD * 2, 16 * st + 4 * hh, 16 * st + 8 + 4 * hh, 32 * c, lane);
            qT[pl] = tr16_frag(qimg + pl * IMG, HD * 2, 16 * st + 4 * hh, 16 * st + 8 + 4 * hh, 32 * c, lane);
          }
          dv[c] = mfma_terms<TERMS>(oT, pB[st], dv[c]);
          dk[c] = mfma_terms<TERMS>(qT, sB[st], dk[c]);
        }
      // dQ^T += K^T dS^T  (k = key, natural order)
      f32x16 dq[NB(HD)];
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[c][r] = 0.f;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        u32x4 sT[3];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
          sT[pl] = tr16_frag(simg + pl * SIMG, 64, 16 * st + 8 * hh, 16 * st + 8 * hh + 4, 0, lane);
#pragma unroll
        for (int c = 0; c < NB(HD); ++c) {
          u32x4 kT[3];
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl)
            kT[pl] = tr16_frag(kimg + pl * IMG, HD * 2, 16 * st + 8 * hh, 16 * st + 8 * hh + 4, 32 * c, lane);
          dq[c] = mfma_terms<TERMS>(kT, sT, dq[c]);
        }
      }
      __builtin_amdgcn_wave_barrier();                   // the images are rewritten by the next pair
      if (jq < K) {                                      // the running dQ partial (single owner)
        float* dqrow = p.dqkv + (tok0 + qrow(jq)) * p.ld + h * HD + 4 * hh;
#pragma unroll
        for (int c = 0; c < NB(HD); ++c)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int dd = 32 * c + 8 * g;
            f32x4 v = {dq[c][4 * g], dq[c][4 * g + 1], dq[c][4 * g + 2], dq[c][4 * g + 3]};
            if (kb > 0) v = *reinterpret_cast<const f32x4*>(dqrow + dd) + v;
            *reinterpret_cast<f32x4*>(dqrow + dd) = v;
          }
      }
    }
    if (kpos < I) {
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = 32 * c + 8 * g + 4 * hh;
          f32x4 a = {dk[c][4 * g], dk[c][4 * g + 1], dk[c][4 * g + 2], dk[c][4 * g + 3]};
          f32x4 v = {dv[c][4 * g], dv[c][4 * g + 1], dv[c][4 * g + 2], dv[c][4 * g + 3]};
          *reinterpret_cast<f32x4*>(dK + (int64_t)kpos * p.ld + dd) = a;
          *reinterpret_cast<f32x4*>(dV + (int64_t)kpos * p.ld + dd) = v;
        }
    }
  }
}

// Key-grouped bf16 backward for long tails (C5: 33 key blocks per (sample, head)).  The per-pair
// kernel above walks every key block with one wave and re-reads the (sample, head)'s Q / dO rows and
// read-modify-writes its dQ rows once per key block — at L = 1036 that is ~70 GB of L2-missing
// traffic per layer.  Here a workgroup of NW waves owns NW consecutive key blocks (one per wave: dK /
// dV accumulators in registers) and streams the query blocks once: each query block's Q / dO rows are
// loaded by the whole workgroup into shared bf16 images (the next block's loads in flight during the
// current block's MFMAs), every wave runs S / dP / softmax gradient / dV / dK for its key block, and
// the NW dQ contributions are summed through LDS in a fixed order and stored once per (slice, query
// block) — slice 0 into dqkv, slice s > 0 into dqpart[s - 1] (attn_dq_reduce_kernel adds them).
// Tail queries only (no selection map), TERMS = 1 (OT_MATMUL_BF16).  NW = ATTN_BWD_GROUP = 4 is the one group
// size built (8 waves, one workgroup per CU, measured slower: attn.h).
// Tried behind compile-time switches and retired with them:
// * XCD-aware slice placement (the S slices of a (sample, head) on one XCD): 4,523 us per C5 layer against 4,489 us
//   without (within noise; the slices' Q / dO re-reads are not the bound).
// * Descending query blocks: every slice of a (sample, head) then streams the same query block at once (with the XCD
//   placement the slices share one L2; the kernel re-reads Q / dO once per slice, ~12 GB per C5 layer): 4,330 us
//   against 4,387-4,489 us ascending (runs/r6ab.sh) — not kept: dK / dV would no longer sum the query blocks in the
//   one-wave-per-pair backward's order (bit-identity, test_attn_bwd_key_slices) for ~0.3% of a C5 step.
// * Three workgroups per CU at head_dim 64 (168 VGPRs) spill 344 B per lane: 13.5 ms — two kept.
// Cross-wave dQ (head_dim 64, 4 waves; kept): after a barrier that publishes every wave's dS^T image, wave w forms dQ^T
// tile w & 1 over key blocks 2 (w >> 1) and 2 (w >> 1) + 1 of the group, and waves 2 / 3 hand theirs to waves 0 / 1
// through an 8 KiB buffer (a third barrier) — the [NW][2][4][64][4] f32 buffer (32 KiB) and its reduce pass go, LDS
// 64 -> 40 KiB per workgroup.  C5 layer (tools/attn_c5_bench.py, runs/r6ad.sh): 4,228-4,240 us against 4,405-4,435;
// dQ sums its four key blocks as (kb0 + kb1) + (kb2 + kb3) instead of one fixed-order pass (dK / dV unchanged, bit for
// bit).  head_dim 32 keeps the fixed-order pass.
template <int HD, int NW>
constexpr bool bwdg_dqx() { return HD == 64 && NW == 4; }
template <int HD, int NW>
constexpr int BWDG_LDS() {
  return 2 * 32 * HD * 2 + NW * (32 * HD * 2 + 32 * 32 * 2) + (bwdg_dqx<HD, NW>() ? (NW - 2) * 64 * 16 * 4 : NW * 32 * HD * 4);
}

template <int HD, int NW, bool QB = false>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_group_kernel(AttnArgs p) {
  constexpr bool DQX = bwdg_dqx<HD, NW>();
  static_assert(HD == 64 || HD == 32, "grouped backward: HD 32 or 64");
  constexpr int NS = HD / 16;                          // k-steps over the head dim
  constexpr int IMG = 32 * HD * 2;                     // one [32][HD] bf16 image
  constexpr int SIMG = 32 * 32 * 2;
  constexpr int NT = 64 * NW;
  constexpr int F4 = 32 * HD / 4;                      // float4 per [32][HD] block
  constexpr int PT = (F4 + NT - 1) / NT;               // float4 per thread per operand
  extern __shared__ __attribute__((aligned(16))) char lds_g[];
  // the wave index in a scalar register: the key-block conditions below are wave-uniform branches
  const int t = threadIdx.x, lane = t & 63, li = lane & 31, hh = lane >> 5, w = __builtin_amdgcn_readfirstlane(t >> 6);
  char* qimg = lds_g;                                  // shared [query][dim] images of the query block
  char* oimg = qimg + IMG;
  char* kimg = oimg + IMG + w * (IMG + SIMG);          // this wave's key block (its V fragments stay in registers)
  char* simg = kimg + IMG;                             // this wave's dS^T [key][query]
  float* dqbuf = reinterpret_cast<float*>(lds_g + 2 * IMG + NW * (IMG + SIMG));   // [NW][NB][4][64 lanes][4]
  const int S = p.kslices;
  const int wg = (int)blockIdx.x;
  const int pair = wg / S, slice = wg - pair * S;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K, KP = attn_kpad(K);
  const int64_t tok0 = (int64_t)b * I;
  const float* Q = p.qkv + tok0 * p.ld + h * HD;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  const float* dO = p.dout + (int64_t)b * K * p.d + h * HD;
  const float* lsep = p.delta + (int64_t)pair * KP;
  const float* dltp = p.delta + ((int64_t)p.B * p.H + pair) * KP;
  float* dK = p.dqkv + tok0 * p.ld + p.d + h * HD;
  float* dV = dK + p.d;
  const int nqb = KP / 32;
  const int kb = slice * NW + w;                       // this wave's key block (>= nkb: an idle wave, P = 0)
  const int key0 = 32 * kb;
  const int kpos = key0 + li;
  const uint16_t* Q16 = reinterpret_cast<const uint16_t*>(p.qkv) + tok0 * p.ld + h * HD;
  // this lane's K / V fragments (row li, dims (HD / 2) hh + 8 st ..) for every query block: held in registers
  u32x4 kF[NS], vF[NS];
  if constexpr (QB) {                                  // bf16 operands: the images are copies
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      const int64_t o = (int64_t)kpos * p.ld + (HD / 2) * hh + 8 * st;
      const u32x4 kB = kpos < I ? *reinterpret_cast<const u32x4*>(Q16 + p.d + o) : z;
      const u32x4 vB = kpos < I ? *reinterpret_cast<const u32x4*>(Q16 + 2 * p.d + o) : z;
      *reinterpret_cast<u32x4*>(kimg + gswz<HD * 2>(li, ((HD / 2) * hh + 8 * st) * 2)) = kB;
      kF[st] = kB;
      vF[st] = vB;
    }
  } else {
    float kf[HD / 2], vf[HD / 2];
    load_frag<HD>(kf, Kp, p.ld, kpos, I, hh);          // rows >= I: zeros (masked below)
    load_frag<HD>(vf, V, p.ld, kpos, I, hh);
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      u32x4 kB[3], vB[3];
      split8t<1>(kf + 8 * st, kB);
      split8t<1>(vf + 8 * st, vB);
      *reinterpret_cast<u32x4*>(kimg + gswz<HD * 2>(li, ((HD / 2) * hh + 8 * st) * 2)) = kB[0];
      kF[st] = kB[0];
      vF[st] = vB[0];
    }
  }
  f32x16 dk[NB(HD)], dv[NB(HD)];
#pragma unroll
  for (int c = 0; c < NB(HD); ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[c][r] = 0.f; dv[c][r] = 0.f; }
  int qbs = 32 * slice * NW - q_off;                   // first query block that sees the group's first key
  qbs = qbs < 0 ? 0 : qbs / 32;
  // cooperative Q / dO block loads: thread t takes float4 e = t + NT i of the [32][HD] block
  f32x4 pq[PT], po[PT];
  u32x2 pq16[PT];
  // the block's lse (lanes 0-31) and delta (lanes 32-63), one float per lane, loaded with the Q / dO rows and
  // parked in the wave's dS^T image until the softmax reads them (that image is rewritten only after it)
  float plsd = 0.f;
  auto load_q = [&](int qb) {
    plsd = lane < 32 ? lsep[32 * qb + lane] : dltp[32 * qb + lane - 32];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int e = t + NT * i;
      const int row = e / (HD / 4), c4 = e % (HD / 4);
      const int j = 32 * qb + row;
      const int jj = j < K ? j : K - 1;                // padded queries: a real row (lse = +inf masks it)
      if constexpr (QB)
        pq16[i] = e < F4 ? *reinterpret_cast<const u32x2*>(Q16 + (int64_t)(q_off + jj) * p.ld + 4 * c4) : u32x2{0u, 0u};
      else
        pq[i] = e < F4 ? *reinterpret_cast<const f32x4*>(Q + (int64_t)(q_off + jj) * p.ld + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
      po[i] = e < F4 ? *reinterpret_cast<const f32x4*>(dO + (int64_t)jj * p.d + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store_q = [&]() {
    reinterpret_cast<float*>(simg)[lane] = plsd;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int e = t + NT * i;
      if (e < F4) {
        const int io = gswz<HD * 2>(e / (HD / 4), (e % (HD / 4)) * 8);
        if constexpr (QB) *reinterpret_cast<u32x2*>(qimg + io) = pq16[i];
        else *reinterpret_cast<u32x2*>(qimg + io) = bf16_rne4(pq[i]);
        *reinterpret_cast<u32x2*>(oimg + io) = bf16_rne4(po[i]);
      }
    }
  };
  const int nit = nqb - qbs;
  load_q(qbs);
  for (int it = 0; it < nit; ++it) {
    const int qb = qbs + it;
    const int q0 = 32 * qb;
    store_q();
    __syncthreads();                                   // images of block qb (and the previous reduce done)
    if (it + 1 < nit) load_q(qb + 1);                  // in flight during this block's MFMAs
    // a wave whose key block lies wholly after this query block (or past the end) contributes zeros
    if (key0 > q_off + q0 + 31 || key0 >= I) {
      if constexpr (!DQX) {
#pragma unroll
        for (int c = 0; c < NB(HD); ++c)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(dqbuf + (((w * NB(HD) + c) * 4 + g) * 64 + lane) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
    u32x4 qA[NS][3], oA[NS][3];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      qA[st][0] = *reinterpret_cast<const u32x4*>(qimg + gswz<HD * 2>(li, ((HD / 2) * hh + 8 * st) * 2));
      oA[st][0] = *reinterpret_cast<const u32x4*>(oimg + gswz<HD * 2>(li, ((HD / 2) * hh + 8 * st) * 2));
    }
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      u32x4 kB[3], vB[3];
      kB[0] = kF[st];
      vB[0] = vF[st];
      s = mfma_terms<1>(qA[st], kB, s);                // S: row = query, col = key
      dp = mfma_terms<1>(oA[st], vB, dp);              // dP
    }
    // the causal mask only where the block pair straddles the diagonal (or holds keys past I): a wholly visible
    // pair skips the per-element compare / select (padded queries have lse = +inf: P = 0 either way)
    if (key0 + 31 <= q_off + q0) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(simg) + 8 * g + 4 * hh);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(simg) + 32 + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float P = __expf(s[r] * p.scale - l4[e]);
          s[r] = P;
          dp[r] = P * (dp[r] - d4[e]) * p.scale;        // dS, pre-scaled by 1/sqrt(hd)
        }
      }
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(simg) + 8 * g + 4 * hh);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(simg) + 32 + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e, j = q0 + 8 * g + 4 * hh + e;
          const float ex = __expf(s[r] * p.scale - l4[e]);
          const float P = kpos <= q_off + j ? ex : 0.f;
          s[r] = P;
          dp[r] = P * (dp[r] - d4[e]) * p.scale;        // dS, pre-scaled by 1/sqrt(hd)
        }
      }
    }
    u32x4 pB[2][3], sB[2][3];
    {
      float pv[16], sv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) { pv[r] = s[r]; sv[r] = dp[r]; }
      split8t<1>(pv, pB[0]); split8t<1>(pv + 8, pB[1]);
      split8t<1>(sv, sB[0]); split8t<1>(sv + 8, sB[1]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u32x4 wv = sB[g >> 1][0];
        const u32x2 two = (g & 1) ? u32x2{wv.z, wv.w} : u32x2{wv.x, wv.y};
        *reinterpret_cast<u32x2*>(simg + gswz<64>(li, (8 * g + 4 * hh) * 2)) = two;
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        u32x4 oT[3], qT[3];
        oT[0] = tr16_frag_sw<HD * 2>(oimg, 16 * st + 4 * hh, 16 * st + 8 + 4 * hh, 32 * c, lane);
        qT[0] = tr16_frag_sw<HD * 2>(qimg, 16 * st + 4 * hh, 16 * st + 8 + 4 * hh, 32 * c, lane);
        dv[c] = mfma_terms<1>(oT, pB[st], dv[c]);      // dV^T += dO^T P
        dk[c] = mfma_terms<1>(qT, sB[st], dk[c]);      // dK^T += Q^T dS
      }
    if constexpr (!DQX) {
    f32x16 dq[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[c][r] = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      u32x4 sT[3];
      sT[0] = tr16_frag_sw<64>(simg, 16 * st + 8 * hh, 16 * st + 8 * hh + 4, 0, lane);
#pragma unroll
      for (int c = 0; c < NB(HD); ++c) {
        u32x4 kT[3];
        kT[0] = tr16_frag_sw<HD * 2>(kimg, 16 * st + 8 * hh, 16 * st + 8 * hh + 4, 32 * c, lane);
        dq[c] = mfma_terms<1>(kT, sT, dq[c]);           // dQ^T += K^T dS^T
      }
    }
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(dqbuf + (((w * NB(HD) + c) * 4 + g) * 64 + lane) * 4) =
            f32x4{dq[c][4 * g], dq[c][4 * g + 1], dq[c][4 * g + 2], dq[c][4 * g + 3]};
    }
    }
    // the dQ store of (slice, query block): float4 a = query jq, dims dd .. dd + 3
    auto store_dq = [&](const f32x4& a, int jq, int dd) {
      if (jq < K && dd < HD) {
        const int ps = p.dq_bf16 ? slice : slice - 1;  // dqpart slot (bf16 output: slice 0 too)
        const int64_t pe = ((int64_t)ps * p.B * K + (int64_t)b * K + jq) * p.d + h * HD + dd;
        if (p.dq_part16) {
          *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(p.dqpart) + pe) = bf16_rne4(a);
        } else {
          float* dst = ps < 0 ? p.dqkv + (tok0 + q_off + jq) * p.ld + h * HD + dd : p.dqpart + pe;
          *reinterpret_cast<f32x4*>(dst) = a;
        }
      }
    };
    if constexpr (DQX) {
      __syncthreads();                                 // every wave's dS^T image is in LDS
      const int c = w & 1;
      f32x16 dq;
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int v = 2 * (w >> 1) + j;                // key block v of the group (uniform)
        const int kv0 = 32 * (slice * NW + v);
        if (kv0 > q_off + q0 + 31 || kv0 >= I) continue;   // its dS is zero (no image written)
        const char* kimg_v = lds_g + 2 * IMG + v * (IMG + SIMG);
        const char* simg_v = kimg_v + IMG;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4 sT[3], kT[3];
          sT[0] = tr16_frag_sw<64>(simg_v, 16 * st + 8 * hh, 16 * st + 8 * hh + 4, 0, lane);
          kT[0] = tr16_frag_sw<HD * 2>(kimg_v, 16 * st + 8 * hh, 16 * st + 8 * hh + 4, 32 * c, lane);
          dq = mfma_terms<1>(kT, sT, dq);              // dQ^T (dims 32c ..) += K_v^T dS_v^T
        }
      }
      float* xb = dqbuf;                               // [NW - 2][4][64 lanes][4]: waves w >= 2 -> wave w & 1
      if (w >= 2) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(xb + (((w - 2) * 4 + g) * 64 + lane) * 4) =
              f32x4{dq[4 * g], dq[4 * g + 1], dq[4 * g + 2], dq[4 * g + 3]};
      }
      __syncthreads();
      if (w < 2) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 a = f32x4{dq[4 * g], dq[4 * g + 1], dq[4 * g + 2], dq[4 * g + 3]};
#pragma unroll
          for (int k = 0; k < NW / 2 - 1; ++k)         // fixed order: key-block pairs 1, 2, ...
            a += *reinterpret_cast<const f32x4*>(xb + (((w + 2 * k) * 4 + g) * 64 + lane) * 4);
          store_dq(a, q0 + li, 32 * c + 8 * g + 4 * hh);
        }
      }
    } else {
      __syncthreads();                                 // every wave's dQ contribution is in LDS
      // fixed-order sum over the NW waves: float4 u = (lane, c, g) -> query q0 + (lane & 31), dims
      // 32c + 8g + 4 (lane >> 5) + 0..3; stored once per (slice, query block)
      for (int u = t; u < NB(HD) * 4 * 64; u += NT) {
        const int ln = u & 63, cg = u >> 6, c = cg >> 2, g = cg & 3;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int v = 0; v < NW; ++v) a += *reinterpret_cast<const f32x4*>(dqbuf + (((v * NB(HD) + c) * 4 + g) * 64 + ln) * 4);
        store_dq(a, q0 + (ln & 31), 32 * c + 8 * g + 4 * (ln >> 5));
      }
    }
  }
  if (kpos < I) {
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = 32 * c + 8 * g + 4 * hh;
        if (dd < HD) {
          f32x4 a = {dk[c][4 * g], dk[c][4 * g + 1], dk[c][4 * g + 2], dk[c][4 * g + 3]};
          f32x4 v = {dv[c][4 * g], dv[c][4 * g + 1], dv[c][4 * g + 2], dv[c][4 * g + 3]};
          if (p.dq_bf16) {
            uint16_t* dK16 = reinterpret_cast<uint16_t*>(p.dqkv) + tok0 * p.ld + p.d + h * HD;
            *reinterpret_cast<u32x2*>(dK16 + (int64_t)kpos * p.ld + dd) = bf16_rne4(a);
            *reinterpret_cast<u32x2*>(dK16 + p.d + (int64_t)kpos * p.ld + dd) = bf16_rne4(v);
          } else {
            *reinterpret_cast<f32x4*>(dK + (int64_t)kpos * p.ld + dd) = a;
            *reinterpret_cast<f32x4*>(dV + (int64_t)kpos * p.ld + dd) = v;
          }
        }
      }
  }
}

// dQ of the key-grouped backward: dqkv[q row] += sum over slices s = 1 .. S-1 whose first key block
// (kgroup * s) the query's block sees of dqpart[s - 1] (fixed slice order: deterministic).  One thread
// per float4 of the [B*K, d] tail dQ.
__global__ __launch_bounds__(256) void attn_dq_reduce_kernel(AttnArgs p) {
  const int64_t e4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int64_t n = (int64_t)p.B * p.K * p.d;
  if (e4 >= n) return;
  const int64_t row = e4 / p.d;
  const int col = (int)(e4 - row * p.d);
  const int b = (int)(row / p.K), j = (int)(row - (int64_t)b * p.K);
  const int q_off = p.I - p.K, qb = j / 32;
  const int o = p.dq_bf16 ? 0 : 1;                     // dqpart slot of slice s: s - o
  const uint16_t* part16 = reinterpret_cast<const uint16_t*>(p.dqpart);
  auto part = [&](int64_t i) -> f32x4 {
    if (!p.dq_part16) return *reinterpret_cast<const f32x4*>(p.dqpart + i);
    const u32x2 w = *reinterpret_cast<const u32x2*>(part16 + i);
    return f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                 __uint_as_float(w.y & 0xffff0000u)};
  };
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bool any = false;
  for (int s = 1; s < p.kslices; ++s) {
    const int f = 32 * p.kgroup * s - q_off;           // first query block that sees the slice's first key
    if ((f < 0 ? 0 : f / 32) > qb) break;              // later slices start later still
    acc += part((int64_t)(s - o) * n + e4);
    any = true;
  }
  const int64_t di = ((int64_t)b * p.I + q_off + j) * p.ld + col;
  if (p.dq_bf16) {
    const f32x4 d0 = part(e4);
    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(p.dqkv) + di) = bf16_rne4(any ? d0 + acc : d0);
    return;
  }
  if (!any) return;
  f32x4* dst = reinterpret_cast<f32x4*>(p.dqkv + di);
  *dst = *dst + acc;
}

// ------------------------------------------------------------------------------------------
// Host launchers (attn.h)

// split-bf16: long sequences, with the next key block prefetched (short ones stay on the f32 kernels, which measure
// faster there: profiles/r01/attention_split.md); bf16 mode: one rounded plane, every length
int attn_planes_fwd_launch(const AttnArgs& p, int head_dim, bool one_plane, hipStream_t st) {
  void (*kern)(AttnArgs) = nullptr;
  switch (head_dim) {
    case 32: kern = one_plane ? attn_fwd_split_kernel<32, 1> : attn_fwd_split_kernel<32, 6>; break;
    case 64: kern = one_plane ? attn_fwd_split_kernel<64, 1> : attn_fwd_split_kernel<64, 6>; break;
    case 128: kern = one_plane ? attn_fwd_split_kernel<128, 1> : attn_fwd_split_kernel<128, 6>; break;
    default: return attn_bad_head_dim(head_dim);
  }
  hipLaunchKernelGGL(kern, dim3(ceil_div((int64_t)p.B * p.H, 4)), dim3(256), 0, st, p);
  return OT_OK;
}

// One-plane bf16 MFMA, one wave per (sample, head), 4 waves / block.  The six-term split form of the same kernel
// measured slower than the f32 kernel at hd 32 (1.42 vs 1.34 ms at C2: the pass is latency-bound, not MFMA-bound),
// so split mode keeps the f32 backward.
int attn_bf16_bwd_launch(const AttnArgs& p, int head_dim, bool sel, hipStream_t st) {
  void (*kern)(AttnArgs) = nullptr;
  const int waves = 4;
  int lds = 0;
  switch (head_dim) {
    case 32:
      kern = sel ? attn_bwd_split_kernel<32, 1, true, 4> : attn_bwd_split_kernel<32, 1, false, 4>;
      lds = BWDS_LDS<32, 1>();
      break;
    case 64:
      kern = sel ? attn_bwd_split_kernel<64, 1, true, 4> : attn_bwd_split_kernel<64, 1, false, 4>;
      lds = BWDS_LDS<64, 1>();
      break;
    default: return attn_bad_head_dim(head_dim);
  }
  static std::once_flag lds_once;                      // hd 64: 72 KiB per 4-wave block (> 64 KiB default)
  std::call_once(lds_once, [] {
    for (void (*k)(AttnArgs) : {attn_bwd_split_kernel<32, 1, true, 4>, attn_bwd_split_kernel<32, 1, false, 4>,
                                attn_bwd_split_kernel<64, 1, true, 4>, attn_bwd_split_kernel<64, 1, false, 4>})
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * BWDS_LDS<64, 1>());
    (void)hipGetLastError();
  });
  hipLaunchKernelGGL(kern, dim3(ceil_div((int64_t)p.B * p.H, waves)), dim3(64 * waves), (size_t)waves * lds, st, p);
  return OT_OK;
}

// Key-grouped workgroups (dQ partials in p.dqpart); QB: bf16 qkv operands (p.qkv_bf16)
int attn_kgroup_bwd_launch(const AttnArgs& p, int head_dim, hipStream_t st) {
  constexpr int G = ATTN_BWD_GROUP;
  void (*kern)(AttnArgs) = nullptr;
  size_t lds = 0;
  switch (head_dim) {
    case 32:
      kern = p.qkv_bf16 ? attn_bwd_group_kernel<32, G, true> : attn_bwd_group_kernel<32, G>;
      lds = BWDG_LDS<32, G>();
      break;
    case 64:
      kern = p.qkv_bf16 ? attn_bwd_group_kernel<64, G, true> : attn_bwd_group_kernel<64, G>;
      lds = BWDG_LDS<64, G>();
      break;
    default: return attn_bad_head_dim(head_dim);
  }
  static std::once_flag glds_once;
  std::call_once(glds_once, [] {
    constexpr int most = BWDG_LDS<32, G>() > BWDG_LDS<64, G>() ? BWDG_LDS<32, G>() : BWDG_LDS<64, G>();
    for (void (*k)(AttnArgs) : {attn_bwd_group_kernel<32, G>, attn_bwd_group_kernel<64, G>,
                                attn_bwd_group_kernel<32, G, true>, attn_bwd_group_kernel<64, G, true>})
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    (void)hipGetLastError();
  });
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.kslices)), dim3(64 * G), lds, st, p);
  if (p.kslices > 1 || p.dq_bf16) {
    OT_LAUNCH_CHECK("ot_attn_bwd");
    hipLaunchKernelGGL(attn_dq_reduce_kernel, dim3(ceil_div((int64_t)p.B * p.K * p.d / 4, 256)), dim3(256), 0, st, p);
  }
  return OT_OK;
}

}  // namespace ot
