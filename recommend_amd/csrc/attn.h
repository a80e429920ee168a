// Causal attention with a query tail: what the per-family files share.
//
//   attention.hip         the ot_attn_* exports, the argument checks and the routing (host code only)
//   attention_wave.hip    f32 MFMA, one wave per (sample, head): attn_fwd_kernel, attn_fwd_kv_kernel,
//                         attn_bwd_prep_kernel, attn_bwd_kernel; and the same family over a request's cached K/V
//                         rows (serving, request-grouped training): attn_fwd_cached_kernel, attn_bwd_cached_kernel
//                         and the ot_attn_*_cached* exports
//   attention_tail.hip    short query tails (K <= SMALL_K) on the VALU: attn_fwd_small_kernel, attn_bwd_small_kernel
//   attention_bf16.hip    bf16 planes: attn_fwd_split_kernel, attn_bwd_split_kernel, attn_bwd_group_kernel,
//                         attn_dq_reduce_kernel
//   attention_kv16.hip    the cached forward over a bf16 cache
// Every kernel is instantiated in one file only; another file reaches it through the host launchers declared at the
// end of this header and defined beside the kernels.
//
// Layout: qkv [B*I, ld] token-major (q at col 0, k at col d, v at col 2d, head h at +h*hd);
// o / dO compact [B*K, d]; lse [B, H, K]; dqkv like qkv (dq only on the K tail rows).
#pragma once
#include "common.h"

namespace ot {

struct AttnArgs {
  const float* qkv; int64_t ld; int d;
  const float* o; const float* dout; float* out; float* lse; float* dqkv; float* delta;
  int B, H, I, K;
  float scale;
  const int32_t* qpos;      // kept query positions [B*K] (ot_pyramid_select) or null: I - K + j
  // key-grouped backward (attn_bwd_group_kernel): kslices workgroups per (sample, head), workgroup s
  // owning key blocks kgroup*s .. kgroup*s + kgroup-1; slice 0 writes dQ into dqkv, slice s > 0 into
  // dqpart[s - 1] ([B*K][d]), summed into dqkv by attn_dq_reduce_kernel
  int kslices, kgroup; float* dqpart;
  // OT_ATTN_DQKV_BF16 (key-grouped backward only): dqkv holds bf16 (uint16 bits, ld in elements); every
  // slice s writes its dQ into dqpart[s] and attn_dq_reduce_kernel stores the rounded sum (slice 0 first,
  // then the later slices in order: the f32 path's sum, rounded once)
  int dq_bf16;
  // OT_ATTN_QKV_BF16 (key-grouped backward only): qkv holds bf16 (uint16 bits, ld in elements) — the fp8
  // forward's dequantised operands, which the bf16 backward would round to bf16 anyway
  int qkv_bf16;
  // OT_ATTN_DQ_PART_BF16 (with OT_ATTN_DQKV_BF16): the slices' dQ partials are stored rounded to bf16 (half the
  // partial traffic; summed in f32 by attn_dq_reduce_kernel, then rounded once more)
  int dq_part16;
  // short-tail backward, f32 dqkv (fp16-pair consumers' bounds): max |dQKV| folded in (one float, zeroed by the
  // caller) and the per-row maxima [B*I][3][H] (dQ / dK / dV part per head; the caller zeroes the array)
  float* amax; float* rowmax;
  // key-padding mask (the MASK instantiations only: ot_attn_fwd_masked / ot_attn_bwd_masked): key_valid[b * ldv + j]
  // != 0 when key j of sample b is a real token; query i sees key j iff j <= i and (valid j or j == i)
  const uint8_t* key_valid; int64_t ldv;
};

// position of kept query j (< K) of the sample whose qpos slice is qp (null: the tail rule)
__device__ __forceinline__ int query_pos(const int32_t* qp, int q_off, int j) { return qp ? qp[j] : q_off + j; }

__device__ __forceinline__ int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// Fragment of a [32 rows x HD] operand for a product over HD: lane (li, hh) holds row li,
// dims (HD/2)*hh + s, s < HD/2 (the k permutation).  Rows >= nrows give zeros.
template <int HD>
__device__ __forceinline__ void load_frag(float (&f)[HD / 2], const float* base, int64_t ld, int row,
                                          int nrows, int hh) {
  if (row < nrows) {
    const float* p = base + (int64_t)row * ld + (HD / 2) * hh;
    if constexpr (HD >= 8) {
#pragma unroll
      for (int q = 0; q < HD / 8; ++q) {
        f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * q);
        f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) f[s] = 0.f;
  }
}

template <int HD>
__device__ __forceinline__ f32x16 mm_frag(const float (&a)[HD / 2], const float (&b)[HD / 2]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < HD / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
  return acc;
}

constexpr int NB(int hd) { return (hd + 31) / 32; }

// O^T[d][col] += sum_r X[row(r)][d0 + li] * P[r]   (X rows are the k index of register r)
template <int HD>
__device__ __forceinline__ void acc_xT_p(f32x16 (&acc)[NB(HD)], const float* xbase, int64_t ld, int row0,
                                         int nrows, const f32x16& p, int li, int hh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + acc_row(r, hh);
#pragma unroll
    for (int c = 0; c < NB(HD); ++c) {
      const int dd = 32 * c + li;
      float a = 0.f;
      if (row < nrows && dd < HD) a = xbase[(int64_t)row * ld + dd];
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[r], acc[c], 0, 0, 0);
    }
  }
}

// Per-wave LDS tile [32][HD+4]: a block the wave holds as row fragments (lane li = row li) is
// written once and read transposed (lane li = column) as the A operand of the accumulator-as-
// operand products — no scalar global re-reads inside the MFMA chains.
template <int HD>
constexpr int TLD() { return HD + 4; }

template <int HD>
__device__ __forceinline__ void frag_to_lds(float* tile, const float (&f)[HD / 2], int li, int hh) {
#pragma unroll
  for (int q = 0; q < HD / 8; ++q)
    *reinterpret_cast<f32x4*>(tile + li * TLD<HD>() + (HD / 2) * hh + 4 * q) =
        f32x4{f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
}

// acc[c] (+)= sum_r tile[row(r)][32c + li] * p[r]
template <int HD>
__device__ __forceinline__ void acc_tile_p(f32x16 (&acc)[NB(HD)], const float* tile, const f32x16& p, int li,
                                           int hh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, hh);
#pragma unroll
    for (int c = 0; c < NB(HD); ++c) {
      const int dd = 32 * c + li;
      const float a = dd < HD ? tile[row * TLD<HD>() + dd] : 0.f;
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[r], acc[c], 0, 0, 0);
    }
  }
}

// Fragment as load_frag, but rows >= nrows read row nrows - 1 (finite data that the masks null).
template <int HD>
__device__ __forceinline__ void load_frag_clamped(float (&f)[HD / 2], const float* base, int64_t ld, int row,
                                                  int nrows, int hh) {
  const float* p = base + (int64_t)(row < nrows ? row : nrows - 1) * ld + (HD / 2) * hh;
#pragma unroll
  for (int q = 0; q < HD / 8; ++q) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * q);
    f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
  }
}

// Queries per (b, h) of the backward's row statistics: K rounded up to the 32-query block (attn_bwd_prep_kernel,
// attention_wave.hip, describes the workspace)
__host__ __device__ constexpr int attn_kpad(int K) { return (K + 31) / 32 * 32; }

// waves per workgroup of the one-wave-per-(sample, head) backwards
template <int HD>
constexpr int BWD_WAVES() { return HD >= 128 ? 2 : 4; }

// the most padded queries for which attn_bwd_kernel forms its own row statistics (its FDL instance)
constexpr int FDL_KP = 160;

// the longest query tail of the short-tail kernels (attention_tail.hip)
constexpr int SMALL_K = 4;

// attn_fwd_kv_kernel stages a (sample, head)'s K and V rows in LDS ([round_up(I, 32)][hd + 4] floats each), up to:
constexpr size_t ATTN_KV_LDS_MAX = 80 * 1024;
inline size_t attn_kv_lds_bytes(int I, int head_dim) {
  return 2 * (size_t)((I + 31) / 32 * 32) * (head_dim + 4) * sizeof(float);
}

// waves (key blocks) per workgroup of attn_bwd_group_kernel.  8 measured slower than 4 at C5 (8.66 against 7.19 ms per
// layer; 18.36 ms for the per-pair kernel) and its instances are no longer built.
constexpr int ATTN_BWD_GROUP = 4;

// a row's lane fragment as load_frag's (lane (li, hh): dims (HD/2)*hh + s), from a row pointer; null: zeros
template <int HD>
__device__ __forceinline__ void load_row_frag(float (&f)[HD / 2], const float* row, int hh) {
  if (row) {
    const float* q = row + (HD / 2) * hh;
#pragma unroll
    for (int i = 0; i < HD / 8; ++i) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(q + 4 * i);
      f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) f[s] = 0.f;
  }
}


// ---- host launchers -----------------------------------------------------------------------------------------------
// Each is defined beside the kernels it launches and holds their only instantiations.  A launcher returns OT_OK or
// the "head_dim unsupported" failure of an instance that is not built; the launch's own error is left for the
// caller's OT_LAUNCH_CHECK, under the caller's label.
inline int attn_bad_head_dim(int head_dim) {
  return fail(OT_ERR_UNSUPPORTED, "attention: head_dim %d unsupported", head_dim);
}

// attention_wave.hip
int attn_wave_fwd_launch(const AttnArgs& p, int head_dim, bool mask, hipStream_t st);   // attn_fwd_kernel<HD, MASK>
int attn_kv_fwd_launch(const AttnArgs& p, int head_dim, hipStream_t st);                // attn_fwd_kv_kernel<HD>
// lse (p.lse) and delta = rowsum(p.dout * p.o) of B x H x K rows, padded, into p.delta (+ the padded p.qpos)
void attn_bwd_prep_launch(const AttnArgs& p, int head_dim, hipStream_t st);
// attn_bwd_kernel<HD, SEL, DS, FDL, MASK>; head_dim 64 runs as two 32-dim waves (DS = 2).  fdl: head_dim 32, tail
// queries, no mask, attn_kpad(K) <= FDL_KP — the one launch that needs no attn_bwd_prep_launch before it
int attn_wave_bwd_launch(const AttnArgs& p, int head_dim, bool sel, bool mask, bool fdl, hipStream_t st);

// attention_tail.hip: K <= SMALL_K (K = 1 takes the one-query instances); the backward after attn_bwd_prep_launch
int attn_tail_fwd_launch(const AttnArgs& p, int head_dim, bool mask, hipStream_t st);
int attn_tail_bwd_launch(const AttnArgs& p, int head_dim, bool mask, hipStream_t st);

// attention_bf16.hip: the backwards after attn_bwd_prep_launch
int attn_planes_fwd_launch(const AttnArgs& p, int head_dim, bool one_plane, hipStream_t st);   // attn_fwd_split_kernel
int attn_bf16_bwd_launch(const AttnArgs& p, int head_dim, bool sel, hipStream_t st);           // attn_bwd_split_kernel
// attn_bwd_group_kernel over p.kslices slices of p.kgroup = ATTN_BWD_GROUP key blocks, then attn_dq_reduce_kernel
// when there are partials to sum (more than one slice, or bf16 dqkv)
int attn_kgroup_bwd_launch(const AttnArgs& p, int head_dim, hipStream_t st);

}  // namespace ot
