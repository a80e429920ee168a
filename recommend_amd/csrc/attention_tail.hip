// Causal attention for a short query tail (K <= SMALL_K: the last layer's one query after DCE) on the VALU:
// attn_fwd_small_kernel and attn_bwd_small_kernel.  attention.hip routes a call here; attn.h has the layout.
#include "attn.h"

namespace ot {

// Backward for a short query tail (K <= SMALL_K, e.g. the last layer's single query after DCE):
// HBM-bound (read K/V rows, write dK/dV rows), so VALU instead of 32x32 MFMA tiles that would be
// 1/32 occupied.  One wave per (sample, head); HD/4 lanes per key (one float4 of dims each), 64/(HD/4)
// keys per pass; dot products reduced over the key's lanes with xor shuffles.  dQ partials are
// reduced over the wave's key slots at the end.
// KQ: the largest K the instance takes (1: the last layer's one query — a quarter of the registers, so more waves
// per SIMD keep more K / V rows in flight)
// MASK: the key-padding mask (AttnArgs.key_valid), one byte per key slot and pass.
template <int HD, int KQ = SMALL_K, bool MASK = false>
__global__ __launch_bounds__(256) void attn_bwd_small_kernel(AttnArgs p) {
  constexpr int LPK = HD / 4, KPW = 64 / LPK;
  const int lane = threadIdx.x & 63, sub = lane % LPK, slot = lane / LPK;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= p.B * p.H) return;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K;
  const int64_t tok0 = (int64_t)b * I;
  const float* Q = p.qkv + tok0 * p.ld + h * HD + 4 * sub;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  float* dK = p.dqkv + tok0 * p.ld + p.d + h * HD + 4 * sub;
  float* dV = dK + p.d;
  const int32_t* qp = p.qpos ? p.qpos + (int64_t)b * K : nullptr;
  float am = 0.f;                                      // max |stored dK / dV / dQ| (p.amax)
  f32x4 q[KQ], o[KQ], dq[KQ];
  float lse[KQ], delta[KQ];
  int qpos[KQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    q[j] = z; o[j] = z; dq[j] = z; lse[j] = 0.f; delta[j] = 0.f; qpos[j] = -1;
    if (j < K) {
      qpos[j] = query_pos(qp, q_off, j);
      q[j] = *reinterpret_cast<const f32x4*>(Q + (int64_t)qpos[j] * p.ld);
      o[j] = *reinterpret_cast<const f32x4*>(p.dout + ((int64_t)b * K + j) * p.d + h * HD + 4 * sub);
      lse[j] = p.delta[(int64_t)pair * attn_kpad(K) + j];
      delta[j] = p.delta[((int64_t)p.B * p.H + pair) * attn_kpad(K) + j];
    }
  }
  // each pass's K / V rows are loaded one pass ahead (two loads per lane in flight during a pass's math)
  f32x4 kvn = *reinterpret_cast<const f32x4*>(Kp + (int64_t)min(slot, I - 1) * p.ld);
  f32x4 vvn = *reinterpret_cast<const f32x4*>(V + (int64_t)min(slot, I - 1) * p.ld);
  for (int key0 = 0; key0 < I; key0 += KPW) {
    const int key = key0 + slot;
    const bool live = key < I;
    const int64_t ro = (int64_t)(live ? key : 0) * p.ld;
    const f32x4 kv = kvn, vv = vvn;
    if (key0 + KPW < I) {
      const int64_t rn = (int64_t)min(key + KPW, I - 1) * p.ld;
      kvn = *reinterpret_cast<const f32x4*>(Kp + rn);
      vvn = *reinterpret_cast<const f32x4*>(V + rn);
    }
    f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
    bool kval = true;
    if constexpr (MASK) kval = live && p.key_valid[(int64_t)b * p.ldv + key] != 0;
#pragma unroll
    for (int j = 0; j < KQ; ++j) {
      if (j >= K) break;
      float sdot = q[j].x * kv.x + q[j].y * kv.y + q[j].z * kv.z + q[j].w * kv.w;
      float pdot = o[j].x * vv.x + o[j].y * vv.y + o[j].z * vv.z + o[j].w * vv.w;
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) {
        sdot += __shfl_xor(sdot, off, 64);
        pdot += __shfl_xor(pdot, off, 64);
      }
      bool vis = live && key <= qpos[j];
      if constexpr (MASK) vis = vis && (kval || key == qpos[j]);
      const float P = vis ? __expf(sdot * p.scale - lse[j]) : 0.f;
      const float ds = vis ? P * (pdot - delta[j]) * p.scale : 0.f;
      dv += P * o[j];
      dk += ds * q[j];
      dq[j] += ds * kv;
    }
    if (live) {
      if (p.dq_bf16) {                                 // bf16 dqkv (OT_ATTN_DQKV_BF16)
        uint16_t* dK16 = reinterpret_cast<uint16_t*>(p.dqkv) + tok0 * p.ld + p.d + h * HD + 4 * sub;
        *reinterpret_cast<u32x2*>(dK16 + ro) = bf16_rne4(dk);
        *reinterpret_cast<u32x2*>(dK16 + p.d + ro) = bf16_rne4(dv);
      } else {
        *reinterpret_cast<f32x4*>(dK + ro) = dk;
        *reinterpret_cast<f32x4*>(dV + ro) = dv;
      }
    }
    if (p.rowmax || p.amax) {                          // (uniform) magnitude bounds of the stored rows
      float rk = live ? amax4(0.f, dk) : 0.f, rv = live ? amax4(0.f, dv) : 0.f;
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) {
        rk = fmaxf(rk, __shfl_xor(rk, off, 64));
        rv = fmaxf(rv, __shfl_xor(rv, off, 64));
      }
      am = fmaxf(am, fmaxf(rk, rv));
      if (p.rowmax && live && sub == 0) {
        float* rr = p.rowmax + (tok0 + key) * 3 * p.H + h;
        rr[p.H] = rk;
        rr[2 * p.H] = rv;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KQ; ++j) {
    if (j >= K) break;
    f32x4 v = dq[j];
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) {
      v.x += __shfl_xor(v.x, off, 64); v.y += __shfl_xor(v.y, off, 64);
      v.z += __shfl_xor(v.z, off, 64); v.w += __shfl_xor(v.w, off, 64);
    }
    if (slot == 0) {
      if (p.dq_bf16)
        *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(p.dqkv) + (tok0 + qpos[j]) * p.ld + h * HD + 4 * sub) =
            bf16_rne4(v);
      else
        *reinterpret_cast<f32x4*>(p.dqkv + (tok0 + qpos[j]) * p.ld + h * HD + 4 * sub) = v;
    }
    if (p.rowmax || p.amax) {                          // (uniform) the dQ row's bound
      float rq = amax4(0.f, v);
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) rq = fmaxf(rq, __shfl_xor(rq, off, 64));
      am = fmaxf(am, rq);
      if (p.rowmax && slot == 0 && sub == 0) p.rowmax[(tok0 + qpos[j]) * 3 * p.H + h] = rq;
    }
  }
  if (p.amax) amax_flush(p.amax, am);
}

// Forward for a short query tail (K <= SMALL_K: the last layer's single query after DCE), the f32-accurate modes.
// HBM-bound (each K / V row read once; 2 K hd flops per row), so plain f32 FMAs on the VALU: the slice kernel's
// MFMA tiles would be 1/16 occupied and it would split all I K / V rows into planes for one query (as slow as a
// full layer).  One wave per (sample, head); HD/4 lanes per key (one float4 of dims each), 64/(HD/4) key slots
// per pass, each slot with its own online softmax (running max m, sum l, output o; scores in log2 units) over the
// keys it sees; the slots' states are merged at the end with xor shuffles (max, then rescaled sums).  Exact f32
// products — no split.
// MASK: the key-padding mask (AttnArgs.key_valid), one byte per key slot and pass; a slot that saw no key keeps
// m = -inf and merges with weight 0, as a slot past the last key does without the mask.
template <int HD, int KQ = SMALL_K, bool MASK = false>
__global__ __launch_bounds__(256) void attn_fwd_small_kernel(AttnArgs p) {
  constexpr int LPK = HD / 4, KPW = 64 / LPK;
  const int lane = threadIdx.x & 63, sub = lane % LPK, slot = lane / LPK;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= p.B * p.H) return;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K;
  const int64_t tok0 = (int64_t)b * I;
  const float* Q = p.qkv + tok0 * p.ld + h * HD + 4 * sub;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  const int32_t* qp = p.qpos ? p.qpos + (int64_t)b * K : nullptr;
  const float c = p.scale * 1.4426950408889634f;      // scores in log2 units
  f32x4 q[KQ], o[KQ];
  float m[KQ], l[KQ];
  int qpos[KQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    q[j] = z; o[j] = z; m[j] = -INFINITY; l[j] = 0.f; qpos[j] = -1;
    if (j < K) {
      qpos[j] = query_pos(qp, q_off, j);
      q[j] = *reinterpret_cast<const f32x4*>(Q + (int64_t)qpos[j] * p.ld) * c;
    }
  }
  int last = 0;                                        // keys past every query's position are never visible
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < K) last = max(last, qpos[j]);
  f32x4 kvn = *reinterpret_cast<const f32x4*>(Kp + (int64_t)min(slot, last) * p.ld);   // one pass ahead
  f32x4 vvn = *reinterpret_cast<const f32x4*>(V + (int64_t)min(slot, last) * p.ld);
  for (int key0 = 0; key0 <= last; key0 += KPW) {
    const int key = key0 + slot;
    const bool live = key <= last;
    const f32x4 kv = kvn, vv = vvn;
    if (key0 + KPW <= last) {
      const int64_t rn = (int64_t)min(key + KPW, last) * p.ld;
      kvn = *reinterpret_cast<const f32x4*>(Kp + rn);
      vvn = *reinterpret_cast<const f32x4*>(V + rn);
    }
    bool kval = true;
    if constexpr (MASK) kval = live && p.key_valid[(int64_t)b * p.ldv + key] != 0;
#pragma unroll
    for (int j = 0; j < KQ; ++j) {
      if (j >= K) break;
      float s = q[j].x * kv.x + q[j].y * kv.y + q[j].z * kv.z + q[j].w * kv.w;
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) s += __shfl_xor(s, off, 64);
      if (live && key <= qpos[j] && (!MASK || kval || key == qpos[j])) {   // (uniform over the key's lanes)
        const float mn = fmaxf(m[j], s);
        const float corr = __builtin_amdgcn_exp2f(m[j] - mn), e = __builtin_amdgcn_exp2f(s - mn);
        l[j] = l[j] * corr + e;
        o[j] = o[j] * corr + e * vv;
        m[j] = mn;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KQ; ++j) {
    if (j >= K) break;
    // merge the key slots (lanes sub + LPK * slot): max of m, then the rescaled l and o summed
    float mx = m[j];
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const float corr = m[j] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[j] - mx);
    float lt = l[j] * corr;
    f32x4 v = o[j] * corr;
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) {
      lt += __shfl_xor(lt, off, 64);
      v.x += __shfl_xor(v.x, off, 64); v.y += __shfl_xor(v.y, off, 64);
      v.z += __shfl_xor(v.z, off, 64); v.w += __shfl_xor(v.w, off, 64);
    }
    if (slot == 0) {
      *reinterpret_cast<f32x4*>(p.out + ((int64_t)b * K + j) * p.d + h * HD + 4 * sub) = v * (1.f / lt);
      if (sub == 0) p.lse[(int64_t)pair * K + j] = mx * 0.6931471805599453f + __logf(lt);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host launchers (attn.h): one query takes the KQ = 1 instance
template <int HD>
static void tail_fwd_launch(const AttnArgs& p, bool mask, hipStream_t st) {
  void (*kern)(AttnArgs) =
      p.K == 1 ? (mask ? attn_fwd_small_kernel<HD, 1, true> : attn_fwd_small_kernel<HD, 1, false>)
               : (mask ? attn_fwd_small_kernel<HD, SMALL_K, true> : attn_fwd_small_kernel<HD, SMALL_K, false>);
  hipLaunchKernelGGL(kern, dim3(ceil_div((int64_t)p.B * p.H, 4)), dim3(256), 0, st, p);
}

template <int HD>
static void tail_bwd_launch(const AttnArgs& p, bool mask, hipStream_t st) {
  void (*kern)(AttnArgs) =
      p.K == 1 ? (mask ? attn_bwd_small_kernel<HD, 1, true> : attn_bwd_small_kernel<HD, 1, false>)
               : (mask ? attn_bwd_small_kernel<HD, SMALL_K, true> : attn_bwd_small_kernel<HD, SMALL_K, false>);
  hipLaunchKernelGGL(kern, dim3(ceil_div((int64_t)p.B * p.H, 4)), dim3(256), 0, st, p);
}

int attn_tail_fwd_launch(const AttnArgs& p, int head_dim, bool mask, hipStream_t st) {
  switch (head_dim) {
    case 16: tail_fwd_launch<16>(p, mask, st); break;
    case 32: tail_fwd_launch<32>(p, mask, st); break;
    case 64: tail_fwd_launch<64>(p, mask, st); break;
    case 128: tail_fwd_launch<128>(p, mask, st); break;
    default: return attn_bad_head_dim(head_dim);
  }
  return OT_OK;
}

int attn_tail_bwd_launch(const AttnArgs& p, int head_dim, bool mask, hipStream_t st) {
  switch (head_dim) {
    case 16: tail_bwd_launch<16>(p, mask, st); break;
    case 32: tail_bwd_launch<32>(p, mask, st); break;
    case 64: tail_bwd_launch<64>(p, mask, st); break;
    case 128: tail_bwd_launch<128>(p, mask, st); break;
    default: return attn_bad_head_dim(head_dim);
  }
  return OT_OK;
}

}  // namespace ot
