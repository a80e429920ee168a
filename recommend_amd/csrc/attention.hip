// Causal attention with a query tail: the ot_attn_* exports, their argument checks and the routing.  Host code
// only — the kernels live in the per-family files listed in attn.h and are reached through its launchers (the
// slice family through attn_slice.h).
//
// Replaces model.py:100-114 (einsum QK^T / sqrt(hd), band_part causal mask filled with -1e9,
// softmax, einsum PV).  The -1e9 fill equals -inf here because the diagonal is never masked.
// Only the last K queries of a layer with I tokens are computed (pyramid keep / last-layer DCE,
// exact), keys/values cover all I tokens.
//
// Which kernel a call runs is decided in attn_fwd_route and attn_bwd_route and nowhere else: the launching
// functions switch on their result, and the capability and workspace queries ask them too, so a caller sizes its
// workspace by the rule that routes it.
#include <algorithm>
#include <cstdint>

#include "attn.h"
#include "attn_slice.h"

using namespace ot;

// ------------------------------------------------------------------------------------------
// Routing

// head dims of the short-tail forward; the queries below name it where they report what the short tail offers
static bool attn_tail_fwd_head_dim(int head_dim) { return head_dim == 32 || head_dim == 64 || head_dim == 128; }

// Forward routes, first match wins:
//   TAIL       K <= SMALL_K, head_dim 32 / 64 / 128, an f32-accurate mode (f32, split): attn_fwd_small_kernel.
//              Narrower than the backward's tail route, which also takes bf16 mode and head_dim 16.
//   SLICE      split mode and the slice fits LDS (attn_slice_fwd_supported): one workgroup per (sample, head).
//   PLANES     head_dim >= 32 and either bf16 mode (one rounded plane, every length) or split mode with I > 256
//              where SHARED_KV does not apply (three planes): attn_fwd_split_kernel.
//   SHARED_KV  head_dim <= 64, K and V of a (sample, head) fit ATTN_KV_LDS_MAX, at least 3 query blocks:
//              attn_fwd_kv_kernel.
//   WAVE       everything else: attn_fwd_kernel.
enum AttnFwdRoute { ATTN_FWD_TAIL, ATTN_FWD_SLICE, ATTN_FWD_PLANES, ATTN_FWD_SHARED_KV, ATTN_FWD_WAVE };

static AttnFwdRoute attn_fwd_route(int I, int K, int head_dim, int precision) {
  if (precision != OT_MATMUL_BF16 && K <= SMALL_K && attn_tail_fwd_head_dim(head_dim)) return ATTN_FWD_TAIL;
  if (precision == OT_MATMUL_SPLIT_BF16 && attn_slice_fwd_supported(I, K, head_dim)) return ATTN_FWD_SLICE;
  const bool kv_fits = head_dim <= 64 && attn_kv_lds_bytes(I, head_dim) <= ATTN_KV_LDS_MAX && (K + 31) / 32 >= 3;
  if (head_dim >= 32 && (precision == OT_MATMUL_BF16 || (precision == OT_MATMUL_SPLIT_BF16 && !kv_fits && I > 256)))
    return ATTN_FWD_PLANES;
  return kv_fits ? ATTN_FWD_SHARED_KV : ATTN_FWD_WAVE;
}

// key-grouped bf16 backward: long tails only — at C2-like lengths (<= 8 key blocks) the per-pair kernel re-reads
// little and has more parallelism
constexpr int ATTN_BWD_GROUP_MIN_KB = 9;
static int attn_kgroup_slices(int I) { return ((I + 31) / 32 + ATTN_BWD_GROUP - 1) / ATTN_BWD_GROUP; }

extern "C" size_t ot_attn_bwd_workspace_size(int B, int H, int K) {
  return (2 * (size_t)B * H + B) * attn_kpad(K) * sizeof(float);     // lse, delta (+ padded qpos)
}

// the row statistics plus `slots` dQ partials of [B*K, d] floats (the key-grouped backward's slices)
static size_t attn_bwd_ws_bytes(int B, int H, int K, int head_dim, int slots) {
  return ot_attn_bwd_workspace_size(B, H, K) + (size_t)slots * B * K * H * head_dim * sizeof(float);
}

// Backward routes, first match wins.  ws_bytes is the caller's workspace; a capability or size query passes
// ATTN_ANY_WS and gets the route a large enough workspace would take.
//   SLICE   split mode, no bf16 flags, K > SMALL_K, attn_slice_bwd_supported (tail queries only), and ws_bytes >=
//           attn_slice_bwd_min_ws: with less, the slice's long forms would run a starved grid, and the call falls
//           through to FDL / WAVE.
//   FDL     tail queries, head_dim 32, SMALL_K < K, attn_kpad(K) <= FDL_KP, not bf16 mode: attn_bwd_kernel forming its
//           own row statistics (no prep launch).
//   TAIL    K <= SMALL_K, every mode and head_dim (16 included, unlike the forward): attn_bwd_small_kernel.
//   KGROUP  bf16 mode, head_dim 32 / 64, tail queries, at least ATTN_BWD_GROUP_MIN_KB key blocks, and ws_bytes holds
//           the slices' dQ partials (ot_attn_bwd_ex_workspace_size): attn_bwd_group_kernel.  With the small
//           workspace of ot_attn_bwd the call falls through to BF16.
//   BF16    bf16 mode, head_dim 32 / 64: attn_bwd_split_kernel, one plane.
//   WAVE    everything else: attn_bwd_kernel after attn_bwd_prep_kernel.
enum AttnBwdRoute { ATTN_BWD_SLICE, ATTN_BWD_FDL, ATTN_BWD_TAIL, ATTN_BWD_KGROUP, ATTN_BWD_BF16, ATTN_BWD_WAVE };
constexpr size_t ATTN_ANY_WS = SIZE_MAX;

static AttnBwdRoute attn_bwd_route(int B, int H, int I, int K, int head_dim, bool selected, int precision, int flags,
                                   size_t ws_bytes) {
  if (precision == OT_MATMUL_SPLIT_BF16 && flags == 0 && K > SMALL_K &&
      attn_slice_bwd_supported(I, K, head_dim, selected) &&
      (ws_bytes == ATTN_ANY_WS || ws_bytes >= attn_slice_bwd_min_ws(B, H, I, K, head_dim)))   // (it asks the device)
    return ATTN_BWD_SLICE;
  if (!selected && head_dim == 32 && K > SMALL_K && attn_kpad(K) <= FDL_KP && precision != OT_MATMUL_BF16)
    return ATTN_BWD_FDL;
  if (K <= SMALL_K) return ATTN_BWD_TAIL;
  if (precision == OT_MATMUL_BF16 && (head_dim == 32 || head_dim == 64)) {
    if (!selected && (I + 31) / 32 >= ATTN_BWD_GROUP_MIN_KB &&
        ws_bytes >= attn_bwd_ws_bytes(B, H, K, head_dim, attn_kgroup_slices(I) - 1))
      return ATTN_BWD_KGROUP;
    return ATTN_BWD_BF16;
  }
  return ATTN_BWD_WAVE;
}

// ------------------------------------------------------------------------------------------
// Capability and workspace queries: the routes at an unlimited workspace, plus what each query adds

extern "C" int ot_attn_amax_supported(int I, int K, int head_dim, int selected, int precision) {
  // the slice kernels fold max |output| in as they store: bit 1 the forward (O), bit 2 the backward (dQKV, tail
  // queries; its long forms reach I 544 at head_dim 64).  The short-tail backward reports its bound too, at the
  // short-tail forward's head dims (not 16).  Split mode only.
  if (precision != OT_MATMUL_SPLIT_BF16) return 0;
  const AttnBwdRoute bwd = attn_bwd_route(1, 1, I, K, head_dim, selected != 0, precision, 0, ATTN_ANY_WS);
  return (attn_fwd_route(I, K, head_dim, precision) == ATTN_FWD_SLICE ? 1 : 0) |
         (bwd == ATTN_BWD_SLICE || (bwd == ATTN_BWD_TAIL && attn_tail_fwd_head_dim(head_dim)) ? 2 : 0);
}

extern "C" int ot_attn_bwd_dqkv_bf16_supported(int I, int K, int head_dim, int selected, int precision) {
  return attn_bwd_route(1, 1, I, K, head_dim, selected != 0, precision, 0, ATTN_ANY_WS) == ATTN_BWD_KGROUP;
}

extern "C" int ot_attn_bwd_bf16_forms(int I, int K, int head_dim, int selected, int precision) {
  const AttnBwdRoute bwd = attn_bwd_route(1, 1, I, K, head_dim, selected != 0, precision, 0, ATTN_ANY_WS);
  if (bwd == ATTN_BWD_KGROUP) return OT_ATTN_DQKV_BF16 | OT_ATTN_QKV_BF16 | OT_ATTN_DQ_PART_BF16;
  if (bwd == ATTN_BWD_TAIL && K > 0 && attn_tail_fwd_head_dim(head_dim)) return OT_ATTN_DQKV_BF16;
  return 0;
}

extern "C" int ot_attn_slice_supported(int I, int K, int head_dim, int selected) {
  // the slice forward fits, and the backward is the slice's or the short tail's
  const AttnBwdRoute bwd = attn_bwd_route(1, 1, I, K, head_dim, selected != 0, OT_MATMUL_SPLIT_BF16, 0, ATTN_ANY_WS);
  return attn_slice_fwd_supported(I, K, head_dim) && (bwd == ATTN_BWD_SLICE || bwd == ATTN_BWD_TAIL);
}

extern "C" size_t ot_attn_bwd_ex_workspace_size(int B, int H, int I, int K, int head_dim, int selected,
                                                int precision) {
  const bool kgroup = attn_bwd_route(B, H, I, K, head_dim, selected != 0, precision, 0, ATTN_ANY_WS) == ATTN_BWD_KGROUP;
  return attn_bwd_ws_bytes(B, H, K, head_dim, kgroup ? attn_kgroup_slices(I) - 1 : 0);
}

extern "C" size_t ot_attn_bwd_flags_workspace_size(int B, int H, int I, int K, int head_dim, int selected, int flags,
                                                   int precision) {
  const AttnBwdRoute bwd = attn_bwd_route(B, H, I, K, head_dim, selected != 0, precision, flags, ATTN_ANY_WS);
  const int S = bwd == ATTN_BWD_KGROUP ? attn_kgroup_slices(I) : 1;
  const size_t n = attn_bwd_ws_bytes(B, H, K, head_dim, (flags & OT_ATTN_DQKV_BF16) ? S : S - 1);   // bf16 dqkv: slice 0 too
  // the slice backward's dS scratch (two workgroups per CU), when that kernel takes the shape
  if (bwd == ATTN_BWD_SLICE) return std::max(n, attn_slice_bwd_ws_bytes(B, H, I, K, head_dim));
  return n;
}

// ------------------------------------------------------------------------------------------
// Forward

static int attn_fwd_impl(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                         int head_dim, float* out, float* lse, int precision, void* stream, float* amax,
                         float* rowmax = nullptr) {
  OT_REQUIRE(precision == OT_MATMUL_F32 || precision == OT_MATMUL_SPLIT_BF16 || precision == OT_MATMUL_BF16,
             "ot_attn_fwd: unknown precision %d", precision);
  OT_REQUIRE(qkv && out && lse, "ot_attn_fwd: null operand");
  OT_REQUIRE(B >= 0 && H > 0 && I > 0 && K > 0 && K <= I, "ot_attn_fwd: bad sizes B=%d H=%d I=%d K=%d", B, H, I, K);
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * H * head_dim, "ot_attn_fwd: ld must be >= 3d and a multiple of 4");
  if (B == 0) return OT_OK;
  AttnArgs p{qkv, ld, H * head_dim, nullptr, nullptr, out, lse, nullptr, nullptr, B, H, I, K,
             1.f / sqrtf((float)head_dim), qpos};
  hipStream_t st = (hipStream_t)stream;
  switch (attn_fwd_route(I, K, head_dim, precision)) {
    case ATTN_FWD_TAIL:
      OT_TRY(attn_tail_fwd_launch(p, head_dim, /*mask=*/false, st));
      OT_LAUNCH_CHECK("ot_attn_fwd(small)");
      return OT_OK;
    case ATTN_FWD_SLICE:
      return attn_slice_fwd(qkv, ld, B, H, I, K, qpos, head_dim, out, lse, st, amax, rowmax);
    case ATTN_FWD_PLANES:
      OT_TRY(attn_planes_fwd_launch(p, head_dim, /*one_plane=*/precision == OT_MATMUL_BF16, st));
      break;
    case ATTN_FWD_SHARED_KV: OT_TRY(attn_kv_fwd_launch(p, head_dim, st)); break;
    case ATTN_FWD_WAVE: OT_TRY(attn_wave_fwd_launch(p, head_dim, /*mask=*/false, st)); break;
  }
  OT_LAUNCH_CHECK("ot_attn_fwd");
  return OT_OK;
}

extern "C" int ot_attn_fwd(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                           int head_dim, float* out, float* lse, int precision, void* stream) {
  return attn_fwd_impl(qkv, ld, B, H, I, K, qpos, head_dim, out, lse, precision, stream, nullptr);
}

extern "C" int ot_attn_fwd_amax(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                                int head_dim, float* out, float* lse, float* amax, float* rowmax, int precision,
                                void* stream) {
  OT_REQUIRE((amax || rowmax) && (ot_attn_amax_supported(I, K, head_dim, qpos != nullptr, precision) & 1),
             "ot_attn_fwd_amax: the output bound needs the slice forward (split mode, I %d K %d head_dim %d: see "
             "ot_attn_amax_supported)", I, K, head_dim);
  return attn_fwd_impl(qkv, ld, B, H, I, K, qpos, head_dim, out, lse, precision, stream, amax, rowmax);
}

// ------------------------------------------------------------------------------------------
// Backward

static int attn_bwd_impl(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                         int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv,
                         float* delta_ws, size_t ws_bytes, int prec, void* stream, int flags = 0,
                         float* amax = nullptr, float* rowmax = nullptr) {
  OT_REQUIRE(prec == OT_MATMUL_F32 || prec == OT_MATMUL_SPLIT_BF16 || prec == OT_MATMUL_BF16,
             "ot_attn_bwd: unknown precision %d", prec);
  OT_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws, "ot_attn_bwd: null operand");
  OT_REQUIRE(B >= 0 && H > 0 && I > 0 && K > 0 && K <= I, "ot_attn_bwd: bad sizes");
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * H * head_dim, "ot_attn_bwd: bad ld");
  if (B == 0) return OT_OK;
  AttnArgs p{qkv, ld, H * head_dim, out, dout, nullptr, const_cast<float*>(lse), dqkv, delta_ws, B, H, I, K,
             1.f / sqrtf((float)head_dim), qpos};
  hipStream_t st = (hipStream_t)stream;
  const bool sel = qpos != nullptr;
  const AttnBwdRoute route = attn_bwd_route(B, H, I, K, head_dim, sel, prec, flags, ws_bytes);
  if (route == ATTN_BWD_SLICE)
    return attn_slice_bwd(qkv, ld, out, dout, lse, B, H, I, K, head_dim, dqkv, delta_ws, ws_bytes, st, amax, rowmax);
  OT_REQUIRE((!amax && !rowmax) || route == ATTN_BWD_TAIL, "ot_attn_bwd_amax: shape not on the slice / short-tail backward");
  p.amax = amax;
  p.rowmax = rowmax;
  if (route == ATTN_BWD_FDL) {
    OT_TRY(attn_wave_bwd_launch(p, head_dim, sel, /*mask=*/false, /*fdl=*/true, st));
    OT_LAUNCH_CHECK("ot_attn_bwd");
    return OT_OK;
  }
  attn_bwd_prep_launch(p, head_dim, st);
  OT_LAUNCH_CHECK("ot_attn_bwd(prep)");
  p.dq_bf16 = (flags & OT_ATTN_DQKV_BF16) ? 1 : 0;
  switch (route) {
    case ATTN_BWD_TAIL: OT_TRY(attn_tail_bwd_launch(p, head_dim, /*mask=*/false, st)); break;
    case ATTN_BWD_KGROUP:
      // dQ partials of the slices behind the row statistics (the ot_attn_bwd_ex workspace)
      p.kslices = attn_kgroup_slices(I);
      p.kgroup = ATTN_BWD_GROUP;
      p.dqpart = delta_ws + ot_attn_bwd_workspace_size(B, H, K) / sizeof(float);
      p.qkv_bf16 = (flags & OT_ATTN_QKV_BF16) ? 1 : 0;
      p.dq_part16 = (flags & OT_ATTN_DQ_PART_BF16) ? 1 : 0;
      OT_TRY(attn_kgroup_bwd_launch(p, head_dim, st));
      break;
    case ATTN_BWD_BF16: OT_TRY(attn_bf16_bwd_launch(p, head_dim, sel, st)); break;
    default: OT_TRY(attn_wave_bwd_launch(p, head_dim, sel, /*mask=*/false, /*fdl=*/false, st)); break;
  }
  OT_LAUNCH_CHECK("ot_attn_bwd");
  return OT_OK;
}

extern "C" int ot_attn_bwd_amax(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                                int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv,
                                void* workspace, size_t ws_bytes, float* amax, float* rowmax, int precision,
                                void* stream) {
  OT_REQUIRE((amax || rowmax) && (ot_attn_amax_supported(I, K, head_dim, qpos != nullptr, precision) & 2) &&
                 ws_bytes >= ot_attn_bwd_flags_workspace_size(B, H, I, K, head_dim, qpos != nullptr, 0, precision),
             "ot_attn_bwd_amax: the dQKV bound needs the slice backward (split mode, tail queries, I %d K %d head_dim "
             "%d, ot_attn_bwd_flags_workspace_size bytes)", I, K, head_dim);
  return attn_bwd_impl(qkv, ld, out, dout, lse, B, H, I, K, qpos, head_dim, dqkv, (float*)workspace, ws_bytes,
                       precision, stream, 0, amax, rowmax);
}

extern "C" int ot_attn_bwd(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                           int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv,
                           float* delta_ws, int precision, void* stream) {
  return attn_bwd_impl(qkv, ld, out, dout, lse, B, H, I, K, qpos, head_dim, dqkv, delta_ws,
                       ot_attn_bwd_workspace_size(B, H, K), precision, stream);
}

extern "C" int ot_attn_bwd_ex(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                              int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv,
                              void* workspace, size_t ws_bytes, int precision, void* stream) {
  OT_REQUIRE(ws_bytes >= ot_attn_bwd_workspace_size(B, H, K), "ot_attn_bwd_ex: workspace too small");
  return attn_bwd_impl(qkv, ld, out, dout, lse, B, H, I, K, qpos, head_dim, dqkv, (float*)workspace, ws_bytes,
                       precision, stream);
}

extern "C" int ot_attn_bwd_flags(const float* qkv, int64_t ld, const float* out, const float* dout,
                                 const float* lse, int B, int H, int I, int K, const int32_t* qpos, int head_dim,
                                 void* dqkv, int flags, void* workspace, size_t ws_bytes, int precision,
                                 void* stream) {
  OT_REQUIRE(!(flags & ~(OT_ATTN_DQKV_BF16 | OT_ATTN_QKV_BF16 | OT_ATTN_DQ_PART_BF16)),
             "ot_attn_bwd_flags: unknown flags %d", flags);
  OT_REQUIRE(!(flags & OT_ATTN_DQ_PART_BF16) || (flags & OT_ATTN_DQKV_BF16),
             "ot_attn_bwd_flags: OT_ATTN_DQ_PART_BF16 goes with OT_ATTN_DQKV_BF16");
  OT_REQUIRE((flags & ot_attn_bwd_bf16_forms(I, K, head_dim, qpos != nullptr, precision)) == flags,
             "ot_attn_bwd_flags: flags %d not supported at I %d K %d head_dim %d (ot_attn_bwd_bf16_forms)", flags, I,
             K, head_dim);
  OT_REQUIRE(!(flags & OT_ATTN_QKV_BF16) || (ot_attn_bwd_dqkv_bf16_supported(I, K, head_dim, qpos != nullptr, precision) &&
                                             ((uintptr_t)qkv % 16) == 0 && ld % 8 == 0),
             "ot_attn_bwd_flags: OT_ATTN_QKV_BF16 needs the key-grouped bf16 backward, 16-B aligned qkv, ld %% 8 == 0");
  OT_REQUIRE(ws_bytes >= ot_attn_bwd_flags_workspace_size(B, H, I, K, head_dim, qpos != nullptr, flags, precision),
             "ot_attn_bwd_flags: workspace too small");
  OT_REQUIRE(!(flags & OT_ATTN_DQKV_BF16) || ((uintptr_t)dqkv % 8) == 0, "ot_attn_bwd_flags: dqkv alignment");
  return attn_bwd_impl(qkv, ld, out, dout, lse, B, H, I, K, qpos, head_dim, (float*)dqkv, (float*)workspace,
                       ws_bytes, precision, stream, flags);
}

// ------------------------------------------------------------------------------------------
// Key-padding mask (include/onetrans_hip.h, "padding mask").  A masked call runs the f32 families at every shape, for
// both f32-accurate precisions: where the un-masked routing takes the TAIL route, the short-tail kernels; everywhere
// else the WAVE route (attn_fwd_kernel; attn_bwd_prep_kernel + attn_bwd_kernel, head_dim 64 as two 32-dim waves), all
// in their MASK instantiations.  The slice, plane, bf16 and fp8 kernels carry no mask: OT_MATMUL_BF16 is refused.  No
// amax / rowmax is reported.
static int attn_masked_check(const char* who, const void* key_valid, int64_t ldv, int B, int H, int I, int K,
                             int64_t ld, int head_dim, int precision) {
  if (precision == OT_MATMUL_BF16)
    return fail(OT_ERR_UNSUPPORTED, "%s: the padding mask runs the f32-accurate kernels only (OT_MATMUL_F32 / "
                "OT_MATMUL_SPLIT_BF16)", who);
  OT_REQUIRE(precision == OT_MATMUL_F32 || precision == OT_MATMUL_SPLIT_BF16, "%s: unknown precision %d", who, precision);
  OT_REQUIRE(B >= 0 && H > 0 && I > 0 && K > 0 && K <= I, "%s: bad sizes B=%d H=%d I=%d K=%d", who, B, H, I, K);
  OT_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128, "%s: head_dim %d unsupported", who,
             head_dim);
  OT_REQUIRE(ld % 4 == 0 && ld >= 3 * (int64_t)H * head_dim, "%s: ld must be >= 3d and a multiple of 4", who);
  OT_REQUIRE(key_valid && ldv >= I, "%s: key_valid is null or ldv < I", who);
  OT_REQUIRE((int64_t)B * H < (int64_t)1 << 31, "%s: grid too large", who);
  return OT_OK;
}

extern "C" int ot_attn_fwd_masked(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                                  int head_dim, const uint8_t* key_valid, int64_t ldv, float* out, float* lse,
                                  int precision, void* stream) {
  if (int rc = attn_masked_check("ot_attn_fwd_masked", key_valid, ldv, B, H, I, K, ld, head_dim, precision)) return rc;
  OT_REQUIRE(qkv && out && lse, "ot_attn_fwd_masked: null operand");
  if (B == 0) return OT_OK;
  AttnArgs p{qkv, ld, H * head_dim, nullptr, nullptr, out, lse, nullptr, nullptr, B, H, I, K,
             1.f / sqrtf((float)head_dim), qpos};
  p.key_valid = key_valid;
  p.ldv = ldv;
  hipStream_t st = (hipStream_t)stream;
  if (attn_fwd_route(I, K, head_dim, precision) == ATTN_FWD_TAIL) OT_TRY(attn_tail_fwd_launch(p, head_dim, /*mask=*/true, st));
  else OT_TRY(attn_wave_fwd_launch(p, head_dim, /*mask=*/true, st));
  OT_LAUNCH_CHECK("ot_attn_fwd_masked");
  return OT_OK;
}

extern "C" int ot_attn_bwd_masked(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                                  int B, int H, int I, int K, const int32_t* qpos, int head_dim,
                                  const uint8_t* key_valid, int64_t ldv, float* dqkv, float* delta_ws, int precision,
                                  void* stream) {
  if (int rc = attn_masked_check("ot_attn_bwd_masked", key_valid, ldv, B, H, I, K, ld, head_dim, precision)) return rc;
  OT_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws, "ot_attn_bwd_masked: null operand");
  if (B == 0) return OT_OK;
  AttnArgs p{qkv, ld, H * head_dim, out, dout, nullptr, const_cast<float*>(lse), dqkv, delta_ws, B, H, I, K,
             1.f / sqrtf((float)head_dim), qpos};
  p.key_valid = key_valid;
  p.ldv = ldv;
  hipStream_t st = (hipStream_t)stream;
  const bool sel = qpos != nullptr;
  attn_bwd_prep_launch(p, head_dim, st);
  OT_LAUNCH_CHECK("ot_attn_bwd_masked(prep)");
  // delta_ws is ot_attn_bwd_workspace_size bytes; only whether the route is TAIL matters here
  const AttnBwdRoute route = attn_bwd_route(B, H, I, K, head_dim, sel, precision, 0, ot_attn_bwd_workspace_size(B, H, K));
  if (route == ATTN_BWD_TAIL) OT_TRY(attn_tail_bwd_launch(p, head_dim, /*mask=*/true, st));
  else OT_TRY(attn_wave_bwd_launch(p, head_dim, sel, /*mask=*/true, /*fdl=*/false, st));
  OT_LAUNCH_CHECK("ot_attn_bwd_masked");
  return OT_OK;
}
