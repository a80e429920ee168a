// Causal attention with a query tail offset on gfx950 fp32 MFMA (v_mfma_f32_32x32x2_f32).
//
// Replaces model.py:100-114 (einsum QK^T / sqrt(hd), band_part causal mask filled with -1e9,
// softmax, einsum PV).  The -1e9 fill equals -inf here because the diagonal is never masked.
// Only the last K queries of a layer with I tokens are computed (pyramid keep / last-layer DCE,
// exact), keys/values cover all I tokens.
//
// This file: the f32 family, one wave per (sample, head); a block of 4 waves = 4 consecutive (b, h) pairs.  The
// layout and the other families are listed in attn.h; attention.hip routes a call here.  The second half of the file
// is the same family over a request's cached K/V rows, with its ot_attn_*_cached* exports.  (The two halves are one
// translation unit on purpose: compiled apart, ten of the kernels here came out with another register assignment
// and schedule than the single-file build's, the same instructions otherwise.)
//
// Orientation: S^T = K Q^T puts the query on the MFMA column (lane) and keys in registers, so
// P^T (registers) is directly the B operand of O^T = V^T P^T (the accumulator-as-operand idiom,
// cdna_hip_programming.md §3) with the k index of step r = the key held in register r.
#include <mutex>

#include "attn.h"

namespace ot {

// Forward.  Scores are kept in the log2 domain (q pre-scaled by log2(e)/sqrt(hd), one multiply per
// q element) so the online softmax uses v_exp_f32 directly; the causal mask is applied on the
// diagonal key block only (earlier blocks are fully visible); K/V rows past the end read as zeros
// (load_frag's row test) and are removed by the mask.  Two variants were built behind compile-time switches
// and retired with them: branch-free K/V loads from a clamped row (load_frag_clamped, still the Q load),
// and the causal select on every key block.
// MASK: the key-padding mask (AttnArgs.key_valid).  The lanes ballot the key block's 32 validity bytes once and every
// accumulator row tests its key's bit; the causal select then runs on every key block (an earlier block is no longer
// fully visible).  A query may see nothing in a block, or in every block before its own position (a padding prefix),
// so the running maximum can still be -inf after a block: the exponents are then taken against 0 instead (every term
// exp2(-inf) = 0, corr = 0 on an accumulator that is still 0), which keeps -inf - (-inf) out of the online softmax.
// The query's own key is always visible, so m and l are finite and positive by the end of the row.
template <int HD, bool MASK = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) float lds[4][32 * TLD<HD>()];
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  float* tV = lds[threadIdx.x >> 6];
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= p.B * p.H) return;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K;
  const float* Q = p.qkv + (int64_t)b * I * p.ld + h * HD;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  const int32_t* qp = p.qpos ? p.qpos + (int64_t)b * K : nullptr;
  const uint8_t* kvp = nullptr;
  if constexpr (MASK) kvp = p.key_valid + (int64_t)b * p.ldv;
  const int nqb = (K + 31) / 32;
  const float qscale = p.scale * 1.4426950408889634f;   // log2(e) / sqrt(hd)
  for (int qb = 0; qb < nqb; ++qb) {
    const int j = 32 * qb + li;                     // this lane's query (kept index)
    const int qpos = query_pos(qp, q_off, j < K ? j : K - 1);
    float qf[HD / 2];
    load_frag_clamped<HD>(qf, Q, p.ld, qpos, I, hh);
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) qf[s] *= qscale;
    f32x16 oacc[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int last_q = query_pos(qp, q_off, min(32 * qb + 31, K - 1));   // positions ascend
    const int nkb = last_q / 32 + 1;
    const int first_masked = query_pos(qp, q_off, 32 * qb) / 32;       // key blocks >= this may be masked
    for (int kb = 0; kb < nkb; ++kb) {
      const int key0 = 32 * kb;
      float kf[HD / 2], vf[HD / 2];
      load_frag<HD>(kf, Kp, p.ld, key0 + li, I, hh);
      load_frag<HD>(vf, V, p.ld, key0 + li, I, hh);
      frag_to_lds<HD>(tV, vf, li, hh);
      f32x16 s = mm_frag<HD>(kf, qf);               // S^T (log2 units): row = key, col = query
      if constexpr (MASK) {
        const int kk = key0 + li;                     // lanes li and li + 32 read the same byte: bits 0..31 are the block
        const uint32_t vm = (uint32_t)__ballot(kk < I && kvp[kk] != 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = acc_row(r, hh), key = key0 + kr;
          s[r] = (key <= qpos && (((vm >> kr) & 1u) || key == qpos)) ? s[r] : -INFINITY;
        }
      } else if (kb >= first_masked) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          s[r] = (key0 + acc_row(r, hh) <= qpos) ? s[r] : -INFINITY;   // kpos <= qpos < I
      }
      float mloc = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, s[r]);
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
      // un-masked: finite from the first block on (key 0 is visible to every query).  MASK: -inf until the row's first
      // visible key; the exponents below are then taken against 0 (see the kernel's header)
      const float mnew = fmaxf(m, mloc);
      const float msub = MASK && mnew == -INFINITY ? 0.f : mnew;
      const float corr = __builtin_amdgcn_exp2f(m - msub);
      float lsum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[r] - msub);
        s[r] = e;
        lsum += e;
      }
      lsum += __shfl_xor(lsum, 32, 64);
      l = l * corr + lsum;
      m = mnew;
#pragma unroll
      for (int c = 0; c < NB(HD); ++c) oacc[c] *= corr;
      __builtin_amdgcn_wave_barrier();
      acc_tile_p<HD>(oacc, tV, s, li, hh);             // O^T += V^T P^T
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
          if (dd < HD) {
            f32x4 v = {oacc[c][4 * g] * inv, oacc[c][4 * g + 1] * inv, oacc[c][4 * g + 2] * inv,
                       oacc[c][4 * g + 3] * inv};
            *reinterpret_cast<f32x4*>(orow + dd) = v;
          }
        }
      // natural-log lse for the backward: m (log2 units) * ln 2 + ln l
      if (hh == 0) p.lse[((int64_t)b * p.H + h) * K + j] = m * 0.6931471805599453f + __logf(l);
    }
  }
}

// Forward, one workgroup per (sample, head) for short sequences: the (b, h) slice's K and V rows
// are staged in LDS once ([KP][HD+4], zero rows past I) and shared by the 4 waves, each of which
// takes whole query blocks (snake order from the heaviest causal block: balanced).  Every K/V byte
// is read from HBM once (the one-wave-per-head kernel re-reads them for every query block).
template <int HD>
__global__ __launch_bounds__(256) void attn_fwd_kv_kernel(AttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float kv[];   // Ks [KP][LD] then Vs [KP][LD]
  constexpr int LD = TLD<HD>();
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5, wave = threadIdx.x >> 6;
  const int pair = blockIdx.x;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K;
  const int KP = (I + 31) / 32 * 32;
  float* Ks = kv;
  float* Vs = kv + KP * LD;
  const float* Q = p.qkv + (int64_t)b * I * p.ld + h * HD;
  // stage K and V: thread t copies float4 chunks (row, c4) of both, rows >= I zero
  constexpr int C4 = HD / 4;
  for (int i = threadIdx.x; i < KP * C4; i += 256) {
    const int row = i / C4, c = 4 * (i % C4);
    f32x4 kvv = {0.f, 0.f, 0.f, 0.f}, vvv = {0.f, 0.f, 0.f, 0.f};
    if (row < I) {
      const float* src = Q + (int64_t)row * p.ld + c;
      kvv = *reinterpret_cast<const f32x4*>(src + p.d);
      vvv = *reinterpret_cast<const f32x4*>(src + 2 * p.d);
    }
    *reinterpret_cast<f32x4*>(Ks + row * LD + c) = kvv;
    *reinterpret_cast<f32x4*>(Vs + row * LD + c) = vvv;
  }
  __syncthreads();
  const int32_t* qp = p.qpos ? p.qpos + (int64_t)b * K : nullptr;
  const int nqb = (K + 31) / 32;
  const float qscale = p.scale * 1.4426950408889634f;   // log2(e) / sqrt(hd)
  for (int i = 0; i < nqb; ++i) {
    const int slot = (i >> 2) & 1 ? 3 - (i & 3) : (i & 3);   // snake assignment
    if (slot != wave) continue;
    const int qb = nqb - 1 - i;
    const int j = 32 * qb + li;
    const int qpos = query_pos(qp, q_off, j < K ? j : K - 1);
    float qf[HD / 2];
    load_frag<HD>(qf, Q, p.ld, j < K ? qpos : I, I, hh);           // rows >= I: zeros
#pragma unroll
    for (int s2 = 0; s2 < HD / 2; ++s2) qf[s2] *= qscale;
    f32x16 oacc[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int last_q = query_pos(qp, q_off, min(32 * qb + 31, K - 1));
    const int nkb = last_q / 32 + 1;
    const int first_masked = query_pos(qp, q_off, 32 * qb) / 32;
    for (int kb = 0; kb < nkb; ++kb) {
      const int key0 = 32 * kb;
      float kf[HD / 2];
#pragma unroll
      for (int q4 = 0; q4 < HD / 8; ++q4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(Ks + (key0 + li) * LD + (HD / 2) * hh + 4 * q4);
        kf[4 * q4] = v.x; kf[4 * q4 + 1] = v.y; kf[4 * q4 + 2] = v.z; kf[4 * q4 + 3] = v.w;
      }
      f32x16 s = mm_frag<HD>(kf, qf);               // S^T (log2 units): row = key, col = query
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
      acc_tile_p<HD>(oacc, Vs + key0 * LD, s, li, hh);     // O^T += V^T P^T
    }
    if (j < K) {
      const float inv = 1.f / l;
      float* orow = p.out + ((int64_t)b * K + j) * p.d + h * HD;
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = 32 * c + 8 * g + 4 * hh;
          if (dd < HD) {
            f32x4 v = {oacc[c][4 * g] * inv, oacc[c][4 * g + 1] * inv, oacc[c][4 * g + 2] * inv,
                       oacc[c][4 * g + 3] * inv};
            *reinterpret_cast<f32x4*>(orow + dd) = v;
          }
        }
      if (hh == 0) p.lse[((int64_t)b * p.H + h) * K + j] = m * 0.6931471805599453f + __logf(l);
    }
  }
}

// Row statistics of the backward, padded to KP = attn_kpad(K) queries per (b, h) so the main
// kernel reads them as aligned float4 without bounds checks:
//   ws[0 .. BH*KP)       lse  (padding +inf: P = exp(s - inf) = 0 masks the padded queries)
//   ws[BH*KP .. 2*BH*KP) delta[b,h,j] = sum_d dO[b*K+j][h*hd+d] * O[b*K+j][h*hd+d]   (padding 0)
//   (int) ws[2*BH*KP .. +B*KP) kept query positions qpos[b][j] padded with qpos[b][K-1] (only
//   when a selection map is given: the selected-query backward reads them as aligned int4)
// Threads of the first `main` blocks take one float4 of [B*K, d] each (coalesced rows), reduced over
// the hd/4 lanes of a head with shuffles; the remaining blocks fill the padding.
__global__ __launch_bounds__(256) void attn_bwd_prep_kernel(const float* __restrict__ o, const float* __restrict__ dout,
                                                            const float* __restrict__ lse, float* ws, int B, int H,
                                                            int K, int hd, int main_blocks, int pad_blocks,
                                                            const int32_t* __restrict__ qpos) {
  const int d = H * hd, KP = attn_kpad(K);
  const int64_t BHKP = (int64_t)B * H * KP;
  if ((int)blockIdx.x >= main_blocks + pad_blocks) {
    const int64_t e = ((int64_t)blockIdx.x - main_blocks - pad_blocks) * blockDim.x + threadIdx.x;   // [B][KP]
    if (!qpos || e >= (int64_t)B * KP) return;
    const int64_t b = e / KP;
    const int j = (int)(e % KP);
    reinterpret_cast<int32_t*>(ws + 2 * BHKP)[e] = qpos[b * K + (j < K ? j : K - 1)];
    return;
  }
  if ((int)blockIdx.x >= main_blocks) {
    const int pad = KP - K;
    const int64_t e = ((int64_t)blockIdx.x - main_blocks) * blockDim.x + threadIdx.x;   // [B*H][pad]
    if (pad == 0 || e >= (int64_t)B * H * pad) return;
    const int64_t bh = e / pad, j = K + e % pad;
    ws[bh * KP + j] = INFINITY;
    ws[BHKP + bh * KP + j] = 0.f;
    return;
  }
  const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;   // element index in [B*K, d]
  const bool live = i4 < (int64_t)B * K * d;
  float s = 0.f;
  if (live) {
    f32x4 x = *reinterpret_cast<const f32x4*>(o + i4);
    f32x4 y = *reinterpret_cast<const f32x4*>(dout + i4);
    s = x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
  }
  for (int off = (hd >> 3); off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  const int c = (int)(i4 % d);
  if (live && (c % hd) == 0) {
    const int64_t row = i4 / d;
    const int64_t b = row / K, j = row % K;
    const int64_t bh = b * H + c / hd;
    ws[bh * KP + j] = lse[bh * K + j];
    ws[BHKP + bh * KP + j] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Backward, one pass per (sample, head) wave: key blocks outer, the query blocks that see them
// inner.  S and dP are computed with the key on the lane, so P and dS feed dV^T += dO^T P and
// dK^T += Q^T dS directly (dO and Q blocks read transposed from per-wave LDS tiles).  dS (pre-scaled
// by 1/sqrt(hd)) is also written to an LDS tile [query][key] and read back as the B operand of
// dQ^T += K^T dS^T (K block from its LDS tile); the dQ^T accumulator has the query on the lane, so
// the running partial in dqkv is read / written as whole float4 row pieces.  The wave owns its
// (b, h) slice: the first key block (seen by every query) stores, later ones read-modify-write the
// same lanes' addresses.  No atomics, no recompute pass, deterministic.
//
// Padding: rows past the end (keys >= I, queries >= K) read as zeros (load_frag's row test); padded keys
// are removed by the causal select, padded queries by lse = +inf.  Branch-free loads from a clamped
// in-bounds row (load_frag_clamped) were the other arm of a compile-time switch, retired unused.
//
// SEL: queries at selected positions (p.qpos, padded copy in the workspace) instead of the tail.
// DS = 2 (head_dim 2 HD, e.g. 64 as two waves of HD = 32): the two waves of a 128-thread block share
// one (sample, head) and each owns half of its dims — half the dK / dV / dQ accumulators, fragments
// and LDS tiles, so a wave has the HD = 32 kernel's footprint (2 waves / SIMD instead of 1).  S and dP
// are sums over all dims: each wave computes its half's partial and the two partials are summed
// through the wave's dS tile (an LDS exchange, four barriers per (key block, query block) pair); the
// softmax gradient is then computed identically in both waves.
// FDL (DS = 1, tail queries, K <= FDL_KP): the row statistics come from the kernel itself instead of
// attn_bwd_prep_kernel — at the first key block (which every query block sees) the wave forms
// delta = rowsum(dO * O) from the dO block it holds anyway and one read of the O block, and copies the
// block's lse (+inf past K); both go to a per-wave LDS row that the later key blocks read.  The prep
// launch and its re-read of dO disappear (C2: 87 us per layer).
// MASK: the key-padding mask (AttnArgs.key_valid).  The key is on the lane: one byte load per key block, and the
// forward's predicate (key <= query and (valid key or key == query)) selects P before it is used (before exp's
// value can matter: an invisible key's exponent may overflow, and the select drops it).
template <int HD, bool SEL, int DS = 1, bool FDL = false, bool MASK = false>
__global__ __launch_bounds__(DS == 1 ? 64 * BWD_WAVES<HD>() : 64 * DS, 2)   // 2 waves per SIMD
void attn_bwd_kernel(AttnArgs p) {
  static_assert(!FDL || (DS == 1 && !SEL), "attn_bwd_kernel: in-kernel row statistics need DS = 1, tail queries");
  static_assert(!FDL || !MASK, "attn_bwd_kernel: the masked backward takes its row statistics from the prep kernel");
  constexpr int LD = TLD<HD>();
  constexpr int SLD = 36;                  // dS tile row stride (32 keys + pad)
  constexpr int PER_WAVE = 3 * 32 * LD + 32 * SLD;
  constexpr int NW = DS == 1 ? BWD_WAVES<HD>() : DS;  // waves per block
  constexpr int HDF = HD * DS;             // head dim
  static_assert(DS == 1 || (DS == 2 && HD == 32), "attn_bwd_kernel: DS = 2 splits head_dim 64");
  // (HD <= 32: the dQ partial is loaded at the start of a pair; larger HD reads it at the end, as
  // the registers of a live seed would not fit next to the dK / dV accumulators)
  constexpr bool SEED_EARLY = HD <= 32;
  __shared__ __attribute__((aligned(16))) float lds[NW * PER_WAVE];
  __shared__ __attribute__((aligned(16))) float rstat[FDL ? NW * 2 * FDL_KP : 4];   // FDL: [wave][lse | delta][KP]
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  const int wave = threadIdx.x >> 6;
  float* tO = lds + wave * PER_WAVE;                 // dO block   [query][dim]
  float* tQ = tO + 32 * LD;                          // Q block    [query][dim]
  float* tK = tQ + 32 * LD;                          // K block    [key][dim]
  float* tS = tK + 32 * LD;                          // dS block   [query][key]
  const float* tSp = lds + (wave ^ 1) * PER_WAVE + 3 * 32 * LD;   // DS = 2: the partner wave's dS tile
  const int pair = DS == 1 ? blockIdx.x * NW + wave : blockIdx.x;
  const int half = DS == 1 ? 0 : wave;
  if (pair >= p.B * p.H) return;
  const int b = pair / p.H, h = pair % p.H;
  const int I = p.I, K = p.K, q_off = I - K, KP = attn_kpad(K);
  const int64_t tok0 = (int64_t)b * I;
  const int hoff = h * HDF + half * HD;                // this wave's first dim of head h
  const float* Q = p.qkv + tok0 * p.ld + hoff;
  const float* Kp = Q + p.d;
  const float* V = Q + 2 * p.d;
  const float* Qt = Q + (int64_t)q_off * p.ld;
  const float* dO = p.dout + (int64_t)b * K * p.d + hoff;
  const int32_t* qpp = reinterpret_cast<const int32_t*>(p.delta + 2 * (int64_t)p.B * p.H * KP) + (int64_t)b * KP;
  const float* lsep = p.delta + (int64_t)pair * KP;                              // padded lse
  const float* dltp = p.delta + ((int64_t)p.B * p.H + pair) * KP;                // padded delta
  float* dQt = p.dqkv + (tok0 + q_off) * p.ld + hoff;
  float* dK = p.dqkv + tok0 * p.ld + p.d + hoff;
  float* dV = dK + p.d;
  // DS = 2: S / dP partial exchange through the dS tiles ([4 groups][64 lanes] float4, 4 KiB)
  auto exchange = [&](f32x16& v) {
    f32x4* mine = reinterpret_cast<f32x4*>(tS);
    const f32x4* theirs = reinterpret_cast<const f32x4*>(tSp);
#pragma unroll
    for (int g = 0; g < 4; ++g) mine[g * 64 + lane] = f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = theirs[g * 64 + lane];
      // fixed operand order (lower half's partial first): both waves get bit-identical sums
      const f32x4 m4 = {v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
      const f32x4 t4 = half == 0 ? m4 + o : o + m4;
      v[4 * g] = t4.x; v[4 * g + 1] = t4.y; v[4 * g + 2] = t4.z; v[4 * g + 3] = t4.w;
    }
    __syncthreads();                                   // the partner is done reading before the next write
  };
  const int nqb = KP / 32;
  const int nkb = (I + 31) / 32;

  for (int kb = 0; kb < nkb; ++kb) {
    const int key0 = 32 * kb;
    const int kpos = key0 + li;                        // this lane's key
    float kf[HD / 2], vf[HD / 2];
    load_frag<HD>(kf, Kp, p.ld, kpos, I, hh);
    load_frag<HD>(vf, V, p.ld, kpos, I, hh);
    // MASK: this lane's key is seen by the queries at kpos .. khi — every later one when it is a real token, only
    // itself when it is padding (one more compare per score, one register per lane)
    int khi = 0x7fffffff;
    if constexpr (MASK) khi = (kpos < I && p.key_valid[(int64_t)b * p.ldv + kpos] != 0) ? 0x7fffffff : kpos;
    frag_to_lds<HD>(tK, kf, li, hh);
    f32x16 dk[NB(HD)], dv[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) { dk[c][r] = 0.f; dv[c][r] = 0.f; }
    int qb0;                                           // first query block that sees key0
    if constexpr (SEL) {
      qb0 = 0;
      while (qb0 < nqb - 1 && qpp[32 * qb0 + 31] < key0) ++qb0;   // ascending positions, padded
    } else {
      qb0 = key0 - q_off; qb0 = qb0 < 0 ? 0 : qb0 / 32;
    }
    float qf[HD / 2], of[HD / 2];
    auto load_qblock = [&](int q0) {
      if constexpr (SEL) load_frag<HD>(qf, Q, p.ld, q0 + li < K ? qpp[q0 + li] : I, I, hh);
      else load_frag<HD>(qf, Qt, p.ld, q0 + li, K, hh);
      load_frag<HD>(of, dO, p.d, q0 + li, K, hh);
    };
    load_qblock(32 * qb0);
    // Per pair, in issue order (vmcnt stays counted, nothing waits early): this block's row stats and
    // dQ seed loads; S / dP chains on the prefetched q block; the next q block's prefetch; softmax
    // gradient; dV / dK chains; dQ chain; dQ store.
    for (int qb = qb0; qb < nqb; ++qb) {
      const int q0 = 32 * qb;
      f32x4 l4[4], d4[4];
      if constexpr (FDL) {
        float* rl = rstat + wave * 2 * FDL_KP;
        if (kb == 0) {                                 // lane li: query q0 + li, dims (HD / 2) hh ..
          float ofo[HD / 2];
          load_frag<HD>(ofo, p.o + (int64_t)b * K * p.d + hoff, p.d, q0 + li, K, hh);
          float pd = 0.f;
#pragma unroll
          for (int s2 = 0; s2 < HD / 2; ++s2) pd += of[s2] * ofo[s2];
          pd += __shfl_xor(pd, 32, 64);
          const int j = q0 + li;
          if (hh == 0) {
            rl[j] = j < K ? p.lse[(int64_t)pair * K + j] : INFINITY;
            rl[FDL_KP + j] = j < K ? pd : 0.f;
          }
          __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          l4[g] = *reinterpret_cast<const f32x4*>(rl + q0 + 8 * g + 4 * hh);
          d4[g] = *reinterpret_cast<const f32x4*>(rl + FDL_KP + q0 + 8 * g + 4 * hh);
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          l4[g] = *reinterpret_cast<const f32x4*>(lsep + q0 + 8 * g + 4 * hh);
          d4[g] = *reinterpret_cast<const f32x4*>(dltp + q0 + 8 * g + 4 * hh);
        }
      }
      // dQ^T block: lane = query q0 + li, register r = dim 32c + acc_row(r, hh) (4 float4 per lane)
      const int jq = q0 + li;
      float* dqrow = SEL ? p.dqkv + (tok0 + qpp[jq]) * p.ld + hoff + 4 * hh
                         : dQt + (int64_t)(jq < K ? jq : K - 1) * p.ld + 4 * hh;
      f32x16 dq[NB(HD)];
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = 32 * c + 8 * g;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (SEED_EARLY && kb > 0 && dd < HD) v = *reinterpret_cast<const f32x4*>(dqrow + dd);
          dq[c][4 * g] = v.x; dq[c][4 * g + 1] = v.y; dq[c][4 * g + 2] = v.z; dq[c][4 * g + 3] = v.w;
        }
      __builtin_amdgcn_wave_barrier();
      frag_to_lds<HD>(tO, of, li, hh);
      frag_to_lds<HD>(tQ, qf, li, hh);
      f32x16 s = mm_frag<HD>(qf, kf);                  // S: row = query, col = key
      f32x16 dp = mm_frag<HD>(of, vf);                 // dP: row = query, col = key
      if constexpr (DS == 2) {                         // whole-head S and dP from the two halves
        exchange(s);
        exchange(dp);
      }
      if (qb + 1 < nqb) load_qblock(q0 + 32);          // prefetch the next query block
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // selected positions read here, not with the row stats: 16 registers fewer across the S / dP
        // chains (the DS = 2 selected-query variant spilled 19 registers holding them)
        i32x4 qv = {0, 0, 0, 0};
        if constexpr (SEL) qv = *reinterpret_cast<const i32x4*>(qpp + q0 + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e, j = q0 + 8 * g + 4 * hh + e;
          const float ex = __expf(s[r] * p.scale - l4[g][e]);
          const int qposj = SEL ? qv[e] : q_off + j;
          const float P = (kpos <= qposj && (!MASK || qposj <= khi)) ? ex : 0.f;
          s[r] = P;
          dp[r] = P * (dp[r] - d4[g][e]) * p.scale;    // dS, pre-scaled by 1/sqrt(hd)
          tS[(8 * g + 4 * hh + e) * SLD + li] = dp[r];
        }
      }
      __builtin_amdgcn_wave_barrier();
      if constexpr (HD <= 32) {
        // dV^T += dO^T P and dK^T += Q^T dS: all 32 LDS operands read first, then the two chains
        // interleaved (independent accumulators) — no LDS round trip between consecutive MFMAs
        float ao[16], aq[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(r, hh);
          ao[r] = li < HD ? tO[row * LD + li] : 0.f;
          aq[r] = li < HD ? tQ[row * LD + li] : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);             // keep the reads above: the scheduler sinks them
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dv[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[r], s[r], dv[0], 0, 0, 0);
          dk[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[r], dp[r], dk[0], 0, 0, 0);
        }
        float bk[16];
        f32x4 a4[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) a4[q4] = *reinterpret_cast<const f32x4*>(tS + li * SLD + 16 * hh + 4 * q4);
#pragma unroll
        for (int e = 0; e < 16; ++e) bk[e] = li < HD ? tK[(16 * hh + e) * LD + li] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
        // dQ^T[d][q] += sum_key K[key][d] dS[q][key]: A = K^T (row = dim, k = key, from tK),
        // B = dS^T (k = key 16hh + s, col = query = lane, from tS)
#pragma unroll
        for (int e = 0; e < 16; ++e) dq[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(bk[e], a4[e >> 2][e & 3], dq[0], 0, 0, 0);
      } else {
        acc_tile_p<HD>(dv, tO, s, li, hh);             // dV^T += dO^T P
        acc_tile_p<HD>(dk, tQ, dp, li, hh);            // dK^T += Q^T dS
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(tS + li * SLD + 16 * hh + 4 * q4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = 16 * hh + 4 * q4 + e;
#pragma unroll
            for (int c = 0; c < NB(HD); ++c) {
              const int dd = 32 * c + li;
              const float bkv = dd < HD ? tK[key * LD + dd] : 0.f;
              dq[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(bkv, a4[e], dq[c], 0, 0, 0);
            }
          }
        }
      }
      if (jq < K) {                                      // the running dQ partial
#pragma unroll
        for (int c = 0; c < NB(HD); ++c)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int dd = 32 * c + 8 * g;
            if (dd >= HD) continue;
            f32x4 v = {dq[c][4 * g], dq[c][4 * g + 1], dq[c][4 * g + 2], dq[c][4 * g + 3]};
            if (!SEED_EARLY && kb > 0) v = *reinterpret_cast<const f32x4*>(dqrow + dd) + v;
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
          if (dd < HD) {
            f32x4 a = {dk[c][4 * g], dk[c][4 * g + 1], dk[c][4 * g + 2], dk[c][4 * g + 3]};
            f32x4 v = {dv[c][4 * g], dv[c][4 * g + 1], dv[c][4 * g + 2], dv[c][4 * g + 3]};
            *reinterpret_cast<f32x4*>(dK + (int64_t)kpos * p.ld + dd) = a;
            *reinterpret_cast<f32x4*>(dV + (int64_t)kpos * p.ld + dd) = v;
          }
        }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host launchers (attn.h)

template <bool MASK>
static int wave_fwd_launch(const AttnArgs& p, int head_dim, hipStream_t st) {
  const dim3 grid(ceil_div((int64_t)p.B * p.H, 4));
  switch (head_dim) {
    case 16: hipLaunchKernelGGL((attn_fwd_kernel<16, MASK>), grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL((attn_fwd_kernel<32, MASK>), grid, dim3(256), 0, st, p); break;
    case 64: hipLaunchKernelGGL((attn_fwd_kernel<64, MASK>), grid, dim3(256), 0, st, p); break;
    case 128: hipLaunchKernelGGL((attn_fwd_kernel<128, MASK>), grid, dim3(256), 0, st, p); break;
    default: return attn_bad_head_dim(head_dim);
  }
  return OT_OK;
}

int attn_wave_fwd_launch(const AttnArgs& p, int head_dim, bool mask, hipStream_t st) {
  return mask ? wave_fwd_launch<true>(p, head_dim, st) : wave_fwd_launch<false>(p, head_dim, st);
}

int attn_kv_fwd_launch(const AttnArgs& p, int head_dim, hipStream_t st) {
  static std::once_flag once;
  std::call_once(once, [] {
    for (const void* k : {(const void*)attn_fwd_kv_kernel<16>, (const void*)attn_fwd_kv_kernel<32>,
                          (const void*)attn_fwd_kv_kernel<64>})
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_KV_LDS_MAX);
    (void)hipGetLastError();
  });
  const size_t kv_bytes = attn_kv_lds_bytes(p.I, head_dim);
  const dim3 grid(p.B * p.H);
  switch (head_dim) {
    case 16: hipLaunchKernelGGL(attn_fwd_kv_kernel<16>, grid, dim3(256), kv_bytes, st, p); break;
    case 32: hipLaunchKernelGGL(attn_fwd_kv_kernel<32>, grid, dim3(256), kv_bytes, st, p); break;
    case 64: hipLaunchKernelGGL(attn_fwd_kv_kernel<64>, grid, dim3(256), kv_bytes, st, p); break;
    default: return attn_bad_head_dim(head_dim);
  }
  return OT_OK;
}

void attn_bwd_prep_launch(const AttnArgs& p, int head_dim, hipStream_t st) {
  const int main_blocks = (int)ceil_div((int64_t)p.B * p.K * p.H * head_dim / 4, 256);
  const int pad_blocks = (int)ceil_div((int64_t)p.B * p.H * (attn_kpad(p.K) - p.K), 256);
  const int qpos_blocks = p.qpos ? (int)ceil_div((int64_t)p.B * attn_kpad(p.K), 256) : 0;
  hipLaunchKernelGGL(attn_bwd_prep_kernel, dim3(main_blocks + pad_blocks + qpos_blocks), dim3(256), 0, st, p.o, p.dout,
                     p.lse, p.delta, p.B, p.H, p.K, head_dim, main_blocks, pad_blocks, p.qpos);
}

template <bool SEL, bool MASK>
static int wave_bwd_launch(const AttnArgs& p, int head_dim, hipStream_t st) {
  void (*kern)(AttnArgs) = nullptr;
  switch (head_dim) {
    case 16: kern = attn_bwd_kernel<16, SEL, 1, false, MASK>; break;
    case 32: kern = attn_bwd_kernel<32, SEL, 1, false, MASK>; break;
    case 64:   // two 32-dim waves per (sample, head): 2 waves / SIMD instead of 1
      hipLaunchKernelGGL((attn_bwd_kernel<32, SEL, 2, false, MASK>), dim3((unsigned)((int64_t)p.B * p.H)), dim3(128), 0, st, p);
      return OT_OK;
    case 128: kern = attn_bwd_kernel<128, SEL, 1, false, MASK>; break;
    default: return attn_bad_head_dim(head_dim);
  }
  const int waves = head_dim >= 128 ? 2 : 4;
  hipLaunchKernelGGL(kern, dim3(ceil_div((int64_t)p.B * p.H, waves)), dim3(64 * waves), 0, st, p);
  return OT_OK;
}

int attn_wave_bwd_launch(const AttnArgs& p, int head_dim, bool sel, bool mask, bool fdl, hipStream_t st) {
  if (fdl) {   // head_dim 32, tail queries, no mask: row statistics formed in the kernel
    hipLaunchKernelGGL((attn_bwd_kernel<32, false, 1, true>), dim3(ceil_div((int64_t)p.B * p.H, BWD_WAVES<32>())),
                       dim3(64 * BWD_WAVES<32>()), 0, st, p);
    return OT_OK;
  }
  if (mask) return sel ? wave_bwd_launch<true, true>(p, head_dim, st) : wave_bwd_launch<false, true>(p, head_dim, st);
  return sel ? wave_bwd_launch<true, false>(p, head_dim, st) : wave_bwd_launch<false, false>(p, head_dim, st);
}

}  // namespace ot

// ==========================================================================================
// Attention over a request's cached K/V rows: the serving forward, and the forward with lse and the backward of
// request-grouped training (the ot_attn_*_cached* exports).  The same family — f32 MFMA, one wave per (candidate,
// head), the fragment helpers of attn.h — and the backward runs attn_bwd_kernel on a candidate's own rows.
namespace ot {

// Serving (paper §3.5.1 two-stage KV cache; the reference's broken cache path model.py:94-98,
// 359-381): candidate c of request req[c] attends with its last Kq N-side queries over the request's
// cached S-side keys/values (Ic rows, computed once per request) and its own n N-side rows.
// Absolute positions: cache rows 0..Ic-1, N rows Ic..Ic+n-1; query j sits at Ic + n - Kq + j, so
// every cached key is visible and the causal mask only touches the N-side key blocks.  Same
// orientation and online softmax as attn_fwd_kernel; key rows come from two sources, so each lane
// resolves its key row's address (one pointer per lane per key block).  ot_attn_fwd_cached writes no lse
// (serving); ot_attn_fwd_cached_lse (request-grouped training) runs the same kernel with the lse output set.
struct AttnCachedArgs {
  const float* qkv; int64_t ld;            // N-side rows [C*n, ld]: q | k | v
  const float* kc; const float* vc; int64_t ldc;   // cached S-side K / V rows [R*Ic, ldc]
  const int32_t* req;                      // [C] request of each candidate
  float* out;                              // [C*Kq, d]
  int C, H, Ic, n, Kq, d;
  float scale;
  float* lse;                              // [C, H, Kq] natural-log row statistics for the backward, or null
  // key-padding mask of the cached rows (the MASK instantiations only): cache_valid[r * ldcv + key], key < Ic; a
  // candidate's own n rows are always valid
  const uint8_t* cache_valid; int64_t ldcv;
};

// MASK: as attn_fwd_kernel's (ballot of the block's validity bits, select on every key block, the -inf guard); the
// queries are N rows, whose own keys are valid, so the predicate needs no self exception.
template <int HD, bool MASK = false>
__global__ __launch_bounds__(256) void attn_fwd_cached_kernel(AttnCachedArgs p) {
  __shared__ __attribute__((aligned(16))) float lds[4][32 * TLD<HD>()];
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  float* tV = lds[threadIdx.x >> 6];
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= p.C * p.H) return;
  const int c = pair / p.H, h = pair % p.H;
  const int Ic = p.Ic, n = p.n, Kq = p.Kq, L = Ic + n;
  const int64_t r = p.req[c];
  const float* Nq = p.qkv + (int64_t)c * n * p.ld + h * HD;        // this candidate's N rows
  const float* Ck = p.kc + r * Ic * p.ldc + h * HD;
  const float* Cv = p.vc + r * Ic * p.ldc + h * HD;
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
      const float* kr = nullptr;
      const float* vr = nullptr;
      if (key < Ic) {
        kr = Ck + (int64_t)key * p.ldc;
        vr = Cv + (int64_t)key * p.ldc;
      } else if (key < L) {
        kr = Nq + (int64_t)(key - Ic) * p.ld + p.d;
        vr = kr + p.d;
      }
      float kf[HD / 2], vf[HD / 2];
      load_row_frag<HD>(kf, kr, hh);
      load_row_frag<HD>(vf, vr, hh);
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
      const float msub = MASK && mnew == -INFINITY ? 0.f : mnew;   // MASK: no visible key yet (attn_fwd_kernel)
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

// ------------------------------------------------------------------------------------------
// Backward of the cached attention (request-grouped training).  A candidate's softmax row runs over the
// request's Ic cached keys and its own n rows; with the row statistics of the whole row (lse, delta) the
// two key ranges are independent sums, so the backward is three passes over disjoint outputs:
//   own rows     attn_bwd_kernel on the candidate's n rows (I = n, K = Kq) with the whole-row lse / delta:
//                dq (own-key part, stored), dk | dv of the n rows.  One wave owns a (candidate, head).
//   cache dK/dV  attn_bwd_cached_kernel<HD, false>: one wave per (request, head, cached key block).  The
//                request's candidates' kept queries are stacked (t = (c - c0) Kq + j) into 32-row query
//                blocks, so c skinny attentions are one dense [c Kq] x Ic problem; the wave walks the
//                stacked blocks in order and is the only writer of its 32 dK / dV rows.
//   cache dQ     attn_bwd_cached_kernel<HD, true>: one workgroup per (request, head), a wave per stacked
//                query block, walking the cached key blocks with P recomputed; the sum is added to the
//                own-rows pass's dq (same stream, one writer per element).
// No atomics, fixed summation order: bit-identical from run to run.  Every cached key is visible, so there
// is no causal select here; padded keys (>= Ic) and padded stacked queries (lse = +inf) give P = 0.
struct AttnCachedBwdArgs {
  const float* qkv; int64_t ld;            // N-side rows [C*n, ld]
  const float* kc; const float* vc; int64_t ldc;
  const int32_t* req_start;                // [R+1]
  const float* dout;                       // [C*Kq, d]
  const float* stat;                       // attn_bwd_prep_kernel's lse | delta, [C*H][KP] each
  float* dqkv; float* dkc; float* dvc;
  int R, C, H, Ic, n, Kq, d, accumulate;
  float scale;
};

template <int HD, bool DQ>
__global__ __launch_bounds__(64 * BWD_WAVES<HD>(), HD >= 128 ? 1 : 2)   // hd 128 needs the whole register file
void attn_bwd_cached_kernel(AttnCachedBwdArgs p) {
  constexpr int LD = TLD<HD>();
  constexpr int SLD = 36;
  constexpr int NW = BWD_WAVES<HD>();
  // per wave: the dK/dV pass holds the dO and Q blocks, the dQ pass the K block and the dS tile
  constexpr int PER_WAVE = (DQ ? 32 * LD + 32 * SLD : 2 * 32 * LD) + 64;
  __shared__ __attribute__((aligned(16))) float lds[NW * PER_WAVE];
  const int lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  const int wave = threadIdx.x >> 6;
  float* tO = lds + wave * PER_WAVE;                 // dO block   [query][dim]   (dK/dV pass)
  float* tQ = tO + 32 * LD;                          // Q block    [query][dim]   (dK/dV pass)
  float* tK = tO;                                    // K block    [key][dim]     (dQ pass)
  float* tS = tK + 32 * LD;                          // dS block   [query][key]   (dQ pass)
  float* rl = lds + wave * PER_WAVE + PER_WAVE - 64; // lse[32] | delta[32] of the query block
  const int Ic = p.Ic, n = p.n, Kq = p.Kq, KP = attn_kpad(Kq);
  const int nkb = (Ic + 31) / 32;
  int r, h, kb_own = 0;
  if constexpr (DQ) {
    r = blockIdx.x / p.H; h = blockIdx.x % p.H;
  } else {
    const int64_t unit = (int64_t)blockIdx.x * NW + wave;
    if (unit >= (int64_t)p.R * p.H * nkb) return;
    kb_own = (int)(unit % nkb);
    const int rh = (int)(unit / nkb);
    r = rh / p.H; h = rh % p.H;
  }
  int c0 = p.req_start[r], c1 = p.req_start[r + 1];
  c0 = min(max(c0, 0), p.C); c1 = min(max(c1, c0), p.C);     // a bad map must not index out of the arrays
  const int Qtot = (c1 - c0) * Kq, nqb = (Qtot + 31) / 32;
  const float* Nq = p.qkv + h * HD;
  const float* dO = p.dout + (int64_t)c0 * Kq * p.d + h * HD;
  const float* Ck = p.kc + (int64_t)r * Ic * p.ldc + h * HD;
  const float* Cv = p.vc + (int64_t)r * Ic * p.ldc + h * HD;
  const float* dlt = p.stat + (int64_t)p.C * p.H * KP;

  float qf[HD / 2], of[HD / 2], kf[HD / 2], vf[HD / 2];
  int64_t qrow = 0;                                    // this lane's query row in [C*n]
  bool qvalid = false;
  // lane li: stacked query 32 qb + li (clamped to the last one; lse = +inf removes the padding)
  auto load_qblock = [&](int qb) {
    const int t = 32 * qb + li;
    qvalid = t < Qtot;
    const int tt = qvalid ? t : Qtot - 1;
    const int cand = c0 + tt / Kq, j = tt % Kq;
    qrow = (int64_t)cand * n + (n - Kq + j);
    load_row_frag<HD>(qf, Nq + qrow * p.ld, hh);
    load_row_frag<HD>(of, dO + (int64_t)tt * p.d, hh);
    const int64_t si = ((int64_t)cand * p.H + h) * KP + j;
    __builtin_amdgcn_wave_barrier();
    if (hh == 0) rl[li] = qvalid ? p.stat[si] : INFINITY;
    else rl[32 + li] = qvalid ? dlt[si] : 0.f;
    if constexpr (!DQ) {
      frag_to_lds<HD>(tO, of, li, hh);
      frag_to_lds<HD>(tQ, qf, li, hh);
    }
    __builtin_amdgcn_wave_barrier();
  };
  // lane li: cached key 32 kb + li (zeros past Ic)
  auto load_kblock = [&](int kb) {
    const int key = 32 * kb + li;
    load_row_frag<HD>(kf, key < Ic ? Ck + (int64_t)key * p.ldc : nullptr, hh);
    load_row_frag<HD>(vf, key < Ic ? Cv + (int64_t)key * p.ldc : nullptr, hh);
    if constexpr (DQ) {
      __builtin_amdgcn_wave_barrier();
      frag_to_lds<HD>(tK, kf, li, hh);
      __builtin_amdgcn_wave_barrier();
    }
  };
  // P (into s) and dS pre-scaled by 1/sqrt(hd) (into dp) of the loaded (query block, key block) pair
  auto softmax_grad = [&](f32x16& s, f32x16& dp, int kb) {
    s = mm_frag<HD>(qf, kf);                           // S: row = query, col = key
    dp = mm_frag<HD>(of, vf);                          // dP: row = query, col = key
    const bool kvalid = 32 * kb + li < Ic;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(rl + 8 * g + 4 * hh);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(rl + 32 + 8 * g + 4 * hh);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = 4 * g + e;
        const float ex = __expf(s[rr] * p.scale - l4[e]);
        const float P = kvalid ? ex : 0.f;
        s[rr] = P;
        dp[rr] = P * (dp[rr] - d4[e]) * p.scale;
      }
    }
  };

  if constexpr (!DQ) {
    const int kpos = 32 * kb_own + li;
    load_kblock(kb_own);
    f32x16 dk[NB(HD)], dv[NB(HD)];
#pragma unroll
    for (int c = 0; c < NB(HD); ++c)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) { dk[c][rr] = 0.f; dv[c][rr] = 0.f; }
    for (int qb = 0; qb < nqb; ++qb) {
      load_qblock(qb);
      f32x16 s, dp;
      softmax_grad(s, dp, kb_own);
      acc_tile_p<HD>(dv, tO, s, li, hh);               // dV^T += dO^T P
      acc_tile_p<HD>(dk, tQ, dp, li, hh);              // dK^T += Q^T dS
    }
    if (kpos < Ic) {
      float* dKr = p.dkc + ((int64_t)r * Ic + kpos) * p.ldc + h * HD;
      float* dVr = p.dvc + ((int64_t)r * Ic + kpos) * p.ldc + h * HD;
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = 32 * c + 8 * g + 4 * hh;
          if (dd < HD) {
            f32x4 a = {dk[c][4 * g], dk[c][4 * g + 1], dk[c][4 * g + 2], dk[c][4 * g + 3]};
            f32x4 v = {dv[c][4 * g], dv[c][4 * g + 1], dv[c][4 * g + 2], dv[c][4 * g + 3]};
            if (p.accumulate) {
              a = *reinterpret_cast<const f32x4*>(dKr + dd) + a;
              v = *reinterpret_cast<const f32x4*>(dVr + dd) + v;
            }
            *reinterpret_cast<f32x4*>(dKr + dd) = a;
            *reinterpret_cast<f32x4*>(dVr + dd) = v;
          }
        }
    }
  } else {
    for (int qb = wave; qb < nqb; qb += NW) {
      load_qblock(qb);
      f32x16 dq[NB(HD)];                               // dQ^T: lane = query, register = dim
#pragma unroll
      for (int c = 0; c < NB(HD); ++c)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) dq[c][rr] = 0.f;
      for (int kb = 0; kb < nkb; ++kb) {
        load_kblock(kb);
        f32x16 s, dp;
        softmax_grad(s, dp, kb);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) tS[(8 * g + 4 * hh + e) * SLD + li] = dp[4 * g + e];
        __builtin_amdgcn_wave_barrier();
        // dQ^T[d][q] += sum_key K[key][d] dS[q][key]
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(tS + li * SLD + 16 * hh + 4 * q4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = 16 * hh + 4 * q4 + e;
#pragma unroll
            for (int c = 0; c < NB(HD); ++c) {
              const int dd = 32 * c + li;
              const float bkv = dd < HD ? tK[key * LD + dd] : 0.f;
              dq[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(bkv, a4[e], dq[c], 0, 0, 0);
            }
          }
        }
      }
      if (qvalid) {                                    // added to the own-rows pass's dq
        float* dqrow = p.dqkv + qrow * p.ld + h * HD + 4 * hh;
#pragma unroll
        for (int c = 0; c < NB(HD); ++c)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int dd = 32 * c + 8 * g;
            if (dd >= HD) continue;
            const f32x4 v = {dq[c][4 * g], dq[c][4 * g + 1], dq[c][4 * g + 2], dq[c][4 * g + 3]};
            *reinterpret_cast<f32x4*>(dqrow + dd) = *reinterpret_cast<const f32x4*>(dqrow + dd) + v;
          }
      }
    }
  }
}

}  // namespace ot

using namespace ot;

// The three forward exports: serving (no lse), request-grouped training (lse required), and either over a masked
// cache (lse optional).  `who` is the export's name in every message.
enum CachedFwd { CACHED_SERVE, CACHED_LSE, CACHED_MASKED };

template <int HD>
static void attn_fwd_cached_launch(const AttnCachedArgs& p, bool masked, hipStream_t st) {
  const dim3 grid(ceil_div((int64_t)p.C * p.H, 4));
  if (masked) hipLaunchKernelGGL((attn_fwd_cached_kernel<HD, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((attn_fwd_cached_kernel<HD, false>), grid, dim3(256), 0, st, p);
}

static int attn_fwd_cached_body(const char* who, CachedFwd kind, const float* qkv, int64_t ld, const float* kv_cache,
                                int64_t ldc, const int32_t* req, int C, int H, int Ic, int n, int Kq, int head_dim,
                                const uint8_t* cache_valid, int64_t ldcv, float* out, float* lse, void* stream) {
  const bool masked = kind == CACHED_MASKED;
  const bool operands = qkv && out && req && (kind != CACHED_LSE || lse) &&
                        (Ic == 0 || (kv_cache && (!masked || (cache_valid && ldcv >= Ic))));
  const char* operands_msg = masked ? "%s: null operand or ldcv < Ic" : "%s: null operand";
  // ot_attn_fwd_cached has always tested its pointers before its sizes, the later two exports after them
  if (kind == CACHED_SERVE) OT_REQUIRE(operands, operands_msg, who);
  OT_REQUIRE(C >= 0 && H > 0 && Ic >= 0 && n > 0 && Kq > 0 && Kq <= n, "%s: bad sizes C=%d Ic=%d n=%d Kq=%d", who, C, Ic,
             n, Kq);
  if (masked)
    OT_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128, "%s: head_dim %d unsupported", who,
               head_dim);
  const int d = H * head_dim;
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * d && (Ic == 0 || (ldc % 4 == 0 && ldc >= 2 * d)),
             "%s: ld/ldc must hold k|v and be multiples of 4", who);
  OT_REQUIRE(operands, operands_msg, who);
  if (C == 0) return OT_OK;
  AttnCachedArgs p{qkv, ld, kv_cache, kv_cache ? kv_cache + d : nullptr, ldc, req, out, C, H, Ic, n, Kq, d,
                   1.f / sqrtf((float)head_dim), lse, cache_valid, ldcv};
  switch (head_dim) {
    case 16: attn_fwd_cached_launch<16>(p, masked, (hipStream_t)stream); break;
    case 32: attn_fwd_cached_launch<32>(p, masked, (hipStream_t)stream); break;
    case 64: attn_fwd_cached_launch<64>(p, masked, (hipStream_t)stream); break;
    case 128: attn_fwd_cached_launch<128>(p, masked, (hipStream_t)stream); break;
    default: return attn_bad_head_dim(head_dim);
  }
  OT_LAUNCH_CHECK(who);
  return OT_OK;
}

extern "C" int ot_attn_fwd_cached(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc,
                                  const int32_t* req, int C, int H, int Ic, int n, int Kq, int head_dim,
                                  float* out, void* stream) {
  return attn_fwd_cached_body("ot_attn_fwd_cached", CACHED_SERVE, qkv, ld, kv_cache, ldc, req, C, H, Ic, n, Kq, head_dim,
                              nullptr, 0, out, nullptr, stream);
}

extern "C" int ot_attn_fwd_cached_lse(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc,
                                      const int32_t* req, int C, int H, int Ic, int n, int Kq, int head_dim,
                                      float* out, float* lse, void* stream) {
  return attn_fwd_cached_body("ot_attn_fwd_cached_lse", CACHED_LSE, qkv, ld, kv_cache, ldc, req, C, H, Ic, n, Kq,
                              head_dim, nullptr, 0, out, lse, stream);
}

extern "C" int ot_attn_fwd_cached_masked(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc,
                                         const int32_t* req, int C, int H, int Ic, int n, int Kq, int head_dim,
                                         const uint8_t* cache_valid, int64_t ldcv, float* out, float* lse_or_null,
                                         void* stream) {
  return attn_fwd_cached_body("ot_attn_fwd_cached_masked", CACHED_MASKED, qkv, ld, kv_cache, ldc, req, C, H, Ic, n, Kq,
                              head_dim, cache_valid, ldcv, out, lse_or_null, stream);
}

extern "C" size_t ot_attn_bwd_workspace_size(int B, int H, int K);

extern "C" size_t ot_attn_bwd_cached_workspace_size(int R, int C, int H, int Ic, int n, int Kq, int head_dim) {
  (void)R; (void)Ic; (void)n; (void)head_dim;
  if (C <= 0 || H <= 0 || Kq <= 0) return 0;
  return ot_attn_bwd_workspace_size(C, H, Kq);                 // padded lse | delta of every (candidate, head)
}

template <int HD>
static void attn_bwd_cached_launch(const AttnCachedBwdArgs& p, hipStream_t stream) {
  constexpr int NW = BWD_WAVES<HD>();
  const int nkb = (p.Ic + 31) / 32;
  hipLaunchKernelGGL((attn_bwd_cached_kernel<HD, false>), dim3((unsigned)ceil_div((int64_t)p.R * p.H * nkb, NW)),
                     dim3(64 * NW), 0, stream, p);
  if (p.C > 0)
    hipLaunchKernelGGL((attn_bwd_cached_kernel<HD, true>), dim3((unsigned)((int64_t)p.R * p.H)), dim3(64 * NW), 0,
                       stream, p);
}

extern "C" int ot_attn_bwd_cached(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc,
                                  const int32_t* req_start, int R, int C, int H, int Ic, int n, int Kq,
                                  int head_dim, const float* out, const float* dout, const float* lse, float* dqkv,
                                  float* dkv_cache, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
  OT_REQUIRE(R >= 0 && C >= 0 && H > 0 && Ic >= 0 && n > 0 && Kq > 0 && Kq <= n,
             "ot_attn_bwd_cached: bad sizes R=%d C=%d Ic=%d n=%d Kq=%d", R, C, Ic, n, Kq);
  OT_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128,
             "ot_attn_bwd_cached: head_dim %d unsupported", head_dim);
  OT_REQUIRE((int64_t)R * H * ((Ic + 31) / 32) < (int64_t)1 << 31 && (int64_t)C * H < (int64_t)1 << 31,
             "ot_attn_bwd_cached: grid too large");
  const int d = H * head_dim;
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * d && (Ic == 0 || (ldc % 4 == 0 && ldc >= 2 * d)),
             "ot_attn_bwd_cached: ld/ldc must hold k|v and be multiples of 4");
  OT_REQUIRE(accumulate == 0 || accumulate == 1, "ot_attn_bwd_cached: accumulate is 0 or 1");
  const size_t need = ot_attn_bwd_cached_workspace_size(R, C, H, Ic, n, Kq, head_dim);
  OT_REQUIRE(ws_bytes >= need, "ot_attn_bwd_cached: workspace too small (%zu < %zu)", ws_bytes, need);
  OT_REQUIRE(qkv && out && dout && lse && dqkv && req_start && (Ic == 0 || (kv_cache && dkv_cache)) &&
                 (need == 0 || workspace), "ot_attn_bwd_cached: null operand");
  hipStream_t st = (hipStream_t)stream;
  const float scale = 1.f / sqrtf((float)head_dim);
  if (C > 0) {
    // row statistics of the whole softmax row, then the candidate's own n rows (the one-wave-per-(sample, head)
    // family over I = n, K = Kq): dq (stored), dk | dv
    AttnArgs a{qkv, ld, d, out, dout, nullptr, const_cast<float*>(lse), dqkv, (float*)workspace, C, H, n, Kq, scale,
               nullptr};
    attn_bwd_prep_launch(a, head_dim, st);
    OT_LAUNCH_CHECK("ot_attn_bwd_cached(prep)");
    OT_TRY(attn_wave_bwd_launch(a, head_dim, /*sel=*/false, /*mask=*/false, /*fdl=*/false, st));
    OT_LAUNCH_CHECK("ot_attn_bwd_cached(own rows)");
  }
  if (Ic == 0 || R == 0) return OT_OK;
  AttnCachedBwdArgs p{qkv, ld, kv_cache, kv_cache + d, ldc, req_start, dout, (const float*)workspace, dqkv,
                      dkv_cache, dkv_cache + d, R, C, H, Ic, n, Kq, d, accumulate, scale};
  switch (head_dim) {
    case 16: attn_bwd_cached_launch<16>(p, st); break;
    case 32: attn_bwd_cached_launch<32>(p, st); break;
    case 64: attn_bwd_cached_launch<64>(p, st); break;
    default: attn_bwd_cached_launch<128>(p, st); break;
  }
  OT_LAUNCH_CHECK("ot_attn_bwd_cached");
  return OT_OK;
}
