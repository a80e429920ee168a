/* onetrans_hip.h — C ABI of libonetrans_hip.so, the gfx950 (MI355X) kernels of the OneTrans
 * ranking training step (fwd + bwd + optimizer).
 *
 * The reference (ScottHCL/recommend, rank/scaling_up/oneTrans/practice) is TensorFlow/Keras with
 * no native code; every entry point below replaces a TF op call site of that model (cited per
 * function as file:line relative to rank/scaling_up/oneTrans/practice/).  The host-side mirror
 * of the reference interface (recommend_amd.OneTransModel / OneTransTrainer) binds this library
 * with ctypes.
 *
 * Conventions
 *  - All tensors are caller-allocated device memory (fp32 activations/weights, int32 row maps,
 *    int64 ids).  The library never allocates, never synchronises the device and keeps no global
 *    mutable state: every call is stream-ordered on `stream` (a hipStream_t passed as void*),
 *    so calls are graph-capturable and thread-safe on distinct streams.
 *  - Scratch memory is passed as (workspace, ws_bytes); size it with the matching
 *    *_workspace_size() function.
 *  - Return 0 (OT_OK) on success, else an OT_ERR_* code; ot_get_last_error_string() describes
 *    the last failure of the calling host thread.
 *  - Row-major 2-D operands are (pointer, leading dimension in elements).  Row maps (int32)
 *    list, per tile row, the source / destination row; -1 marks padding.
 *  - Dropout masks are counter-based: element (token t, column n) of site s is kept iff
 *    fmix32((t*width + n) * 0x9E3779B1 + seed ^ s * 0x85EBCA77) >= rate * 2^32, kept values are
 *    scaled by 1/(1-rate).  A compacted tail row r (the last K of I tokens per sample) maps to
 *    token t = (r / K) * I + (I - K) + r % K, or, when a kept-position map `tail_pos` [B*K]
 *    from ot_pyramid_select is passed, t = (r / K) * I + tail_pos[r].
 */
#ifndef ONETRANS_HIP_H
#define ONETRANS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OT_OK 0
#define OT_ERR_INVALID_ARG 1
#define OT_ERR_UNSUPPORTED 2
#define OT_ERR_HIP 3

/* GEMM modes */
#define OT_GEMM_NN 0 /* C = A @ W[g],   W[g] stored [K][N] (Keras Dense kernel layout) */
#define OT_GEMM_NT 1 /* C = A @ W[g]^T, W[g] stored [N][K] (dgrad through a Keras kernel) */

/* A-load prologues */
#define OT_AX_NONE 0
#define OT_AX_RMSNORM 1 /* a * rstd[in_row] * gamma[k]  (RMSNorm fused into the consumer GEMM) */
#define OT_AX_GELU 2    /* gelu_erf(a)                   (FFN hidden recomputed from its pre-activation) */
#define OT_AX_BF16 4    /* A holds bf16 values (uint16 bits, lda in elements), used as they are (the stored
                           GELU of ot_rms_epilogue.gelu_out).  ot_mixed_gemm_wgrad: OT_MATMUL_BF16 / split
                           modes; forward GEMMs: OT_MATMUL_BF16, NT mode, a B image (the plane GEMM), lda % 8
                           == 0, 16-B aligned A, epilogue OT_EPI_BIAS | OT_EPI_RESIDUAL [| OT_EPI_DROPOUT]
                           [| OT_EPI_ROW_RSTD] (the FFN2 GEMM) */
#define OT_AX_BF16_RMSNORM 5 /* plane GEMM, OT_MATMUL_BF16: A holds bf16 x (as OT_AX_BF16) and the RMSNorm is applied
                                as the RMSNorm prologue is there (gamma folded into the B image, rstd scales the
                                output rows): the QKV / FFN1 GEMMs from the bf16 copy of their input */

/* GEMM epilogue flags (applied in this order) */
#define OT_EPI_BIAS 1        /* + bias[g][n] */
#define OT_EPI_GELU_BWD 2    /* * gelu'(aux[out_row][n]) */
#define OT_EPI_GELU 4        /* gelu_erf(.) */
#define OT_EPI_DROPOUT 8     /* counter-based mask, index (token, n) */
#define OT_EPI_RESIDUAL 16   /* + res[res_tok ? token : out_row][n] */
#define OT_EPI_ACCUMULATE 32 /* C += result */
/* row-norm epilogues (ot_mixed_gemm_rms only): N == 128 (one tile holds whole output rows); OT_EPI_ROW_RSTD
 * also N = 256, 384, ... on the plane GEMM (split mode, ot_mixed_gemm_rms_img; per-tile row sums of
 * squares in the workspace, ot_mixed_gemm_rms_workspace_size(ntiles, N), then a finishing pass);
 * OT_EPI_RMSNORM_BWD also N = 256, 384, ... given the row dots' partials (ot_rms_epilogue.rowdot) */
#define OT_EPI_ROW_RSTD 64      /* rstd_out[out_row] = 1/sqrt(mean_n(C[out_row]^2) + eps), C as above */
#define OT_EPI_ROWDOT 256       /* with OT_EPI_GELU_BWD (ot_mixed_gemm_rms, N % 128 == 0): also
                                   rowdot[out_row * rowdot_n + n / 128] = sum over the tile's columns of
                                   C * (aux - bias[g]) — for the FFN2 dgrad (C = dU, aux = U, bias = b1)
                                   this is the FFN1 norm backward's row dot: sum_f dU_f (U_f - b1_f) =
                                   rstd * <gamma dy, x> (no row-wide reduction needed at d > 128) */
#define OT_EPI_RMSNORM_BWD 128  /* the product is dL/dy of y = RMSNorm(x) * gamma: C = dL/dx (+ dres);
                                   with OT_EPI_DROPOUT also dx_masked = mask(C) (C itself unmasked) */
#define OT_EPI_C_BF16 512       /* C is stored rounded to bf16 (uint16 bits, ldc in elements; 8-B aligned
                                   rows).  Plane GEMM in the bf16 mode, with OT_EPI_GELU_BWD [| OT_EPI_ROWDOT]
                                   [| OT_EPI_AUX_BF16] (the FFN2 dgrad: dU, whose consumers — the FFN1 dgrad
                                   and the W1 weight gradient — round it to bf16 anyway) or with OT_EPI_BIAS
                                   alone (the FFN1 forward: U, read only by the FFN2 dgrad's GELU') */
#define OT_EPI_AUX_BF16 1024    /* with OT_EPI_GELU_BWD: aux holds bf16 (uint16 bits, ldaux in elements) — the
                                   bf16 mode's stored pre-activation U (plane GEMM, OT_MATMUL_BF16 only) */
/* ot_mixed_gemm_wgrad: or'ed into a_xform, D holds bf16 values (uint16 bits, ldd in elements; 8-B aligned
 * rows; OT_MATMUL_BF16 / split modes) — dU stored by OT_EPI_C_BF16 */
#define OT_WG_D_BF16 8
/* ot_mixed_gemm_wgrad_keep: or'ed into a_xform, D is the gradient before a dropout mask and the call's keep bits
 * select and scale it at staging time */
#define OT_WG_D_KEEPBITS 16

int ot_version(void);
const char* ot_get_last_error_string(void);

/* ---- mixed-parameterisation grouped GEMM (gemm.hip: dispatch and the register-staged kernel;
 * gemm_plane.hip, gemm_plane_wide.hip: the plane GEMMs; gemm_images.hip: their weight images;
 * gemm_wgrad.hip: weight gradients) ----------------------------------------------------------
 * Replaces: per-token Q/K/V Dense loop model.py:84-92 (+ weights 38-54, group rule 67-74),
 * Wo model.py:117, per-token FFN loop model.py:154-161 (weights 136-147), tokenizer Dense layers
 * model.py:211-219/254/265, task-head Dense(d/2) model.py:325-330/391, and their gradients
 * (tape.gradient, train.py:131).  Tiles are 128 rows (ot_gemm_tile_rows()); tile i multiplies the
 * rows in_rows[128 i .. 128 i + 127] by W + tile_group[i] * w_gstride. */
int ot_gemm_tile_rows(void);
/* Matmul arithmetic: the `precision` argument of every GEMM, weight-gradient, plane-image and attention
 * entry point (per call: no process-wide state, so models of different precision share the library).
 *   OT_MATMUL_SPLIT_BF16 (default): every f32 operand is split exactly into three bf16 parts
 *     (x = x0 + x1 + x2, 8 significant bits each) and the product is sum_ij ai.bj over the six
 *     largest terms on v_mfma_f32_32x32x16_bf16 (each part product exact in the f32 accumulator;
 *     the dropped a1.b2 + a2.b1 + a2.b2 is below 2^-22 |a||b|, one f32 rounding).  Error vs an
 *     f64 product measured no larger than native f32 (tools/split_gemm_check.py).
 *   OT_MATMUL_F32: native v_mfma_f32_32x32x2_f32.
 *   OT_MATMUL_BF16: reduced precision (BASELINE C5's bf16 configuration, not the reference's f32):
 *     operands rounded to bf16 (nearest even), one v_mfma_f32_32x32x16_bf16 product, f32
 *     accumulation; attention forward and backward likewise.
 * Keras computes these Dense layers in f32 (model.py:38-57, 136-147; default float32 policy). */
#define OT_MATMUL_F32 0
#define OT_MATMUL_SPLIT_BF16 1
#define OT_MATMUL_BF16 2
int ot_mixed_gemm(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                  int a_xform, const float* a_rstd, const float* a_gamma,
                  const float* W, int64_t w_gstride, int64_t ldw, int N,
                  const int32_t* tile_group, int ntiles,
                  const float* bias, int64_t bias_gstride,
                  float* C, int64_t ldc, const int32_t* out_rows, int epi,
                  const float* res, int64_t ldres, int res_tok,
                  const float* aux, int64_t ldaux,
                  uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                  const int32_t* tail_pos, int precision, void* stream);
/* Row-norm epilogue operands for ot_mixed_gemm_rms.  Replaces the RMSNorm layers around the GEMMs
 * (model.py:11-23 RMSNorm, applied at 191/196; their tape gradients): the forward GEMM producing the
 * residual stream emits the next norm's rstd, the dgrad GEMM feeding a norm applies its backward. */
typedef struct ot_rms_epilogue {
  size_t struct_size;                                  /* sizeof(ot_rms_epilogue) of the caller's header: the
                                                          library rejects any other value (OT_ERR_INVALID_ARG)
                                                          instead of reading fields a smaller struct lacks */
  float* rstd_out; float eps;                          /* OT_EPI_ROW_RSTD */
  const float* x; int64_t ldx;                         /* OT_EPI_RMSNORM_BWD: norm input rows (out_row) */
  const float* gamma; const float* rstd;               /*   gamma[N], rstd[out_row] */
  const float* dres; int64_t lddres;                   /*   + dres (row out_row, or through the tail map */
  int dres_tail_K, dres_tail_I;                        /*     b*I+p -> b*K+(p-(I-K)) when dres_tail_K > 0) */
  const int32_t* dres_tail_inv;                        /*     or b*I+p -> inv[b*I+p] (ot_pyramid_select) */
  float* dx_masked; int64_t lddxm;                     /*   with OT_EPI_DROPOUT: GEMM seed/site/rate/tail */
  float* dgamma; int accumulate_dgamma;                /*   dgamma (+)= sum_rows dy * x * rstd */
  void* workspace; size_t ws_bytes;                    /*   ot_mixed_gemm_rms_workspace_size(ntiles, N) */
  float* rowdot; int rowdot_n;                         /* OT_EPI_ROWDOT: output partials [out rows][rowdot_n];
                                                          OT_EPI_RMSNORM_BWD with N > 128: their input (the row
                                                          dot = sum_j rowdot[out_row][j] / rstd) */
  uint16_t* gelu_out; int64_t ldgelu;                  /* optional, whole tiles: also gelu_erf(aux) (with
                                                          OT_EPI_GELU_BWD) or gelu_erf(C) (epi == OT_EPI_BIAS: the
                                                          FFN1 forward, C = U) rounded to bf16 at [out_row][n] —
                                                          the FFN2 GEMM's and its weight gradient's A operand in
                                                          the bf16 mode (OT_AX_BF16): they neither read f32 U nor
                                                          re-evaluate erf.  No other row-norm field is needed */
  uint16_t* xn_out; int64_t ldxn;                      /* optional, with the RMSNorm prologue on the plane GEMM:
                                                          also bf16((A * gamma) * rstd) of every A row [in_row][k]
                                                          (written by the first column tile's workgroups) — the
                                                          normalised operand of the bf16-mode weight gradient
                                                          (OT_AX_BF16), so it neither re-reads f32 A nor
                                                          re-applies the norm */
  uint16_t* c16_out; int64_t ldc16;                    /* optional, bf16-mode plane GEMM (not with the norm-backward
                                                          or bf16-C epilogues): also C rounded to bf16 — the next
                                                          GEMM's OT_AX_BF16_RMSNORM operand */
  float* rowmax_out; int rowmax_n;                     /* optional, split-mode plane GEMM: each 128-column tile's
                                                          largest C value after the bias (signed) at
                                                          [out_row][tile] (rowmax_n = N / 128): the FFN1 forward's
                                                          row maxima of U for the FFN2 GEMM's a_rowmax */
  const float* a_rowmax; int a_rowmax_n;               /* optional, split-mode plane GEMM with the GELU prologue
                                                          (or none: then the parts are max |a|, e.g. rowabs_out /
                                                          ot_dropout_apply_ex / ot_rows_absmax of A's producer):
                                                          the A rows' partial maxima [in_row][a_rowmax_n] (as
                                                          rowmax_out wrote them); the GEMM then multiplies on the
                                                          scaled fp16 pair, the row scale from max(max_j a_rowmax,
                                                          0.17) >= max |gelu(a)|, and b_image must be a pair image
                                                          (desc kscale_off -2, ot_split_images) */
  float* amax_out;                                     /* optional, whole-tile kernels: *amax_out = max(*amax_out,
                                                          max |v|) over the values v the epilogue stores for the next
                                                          consumer (dx_masked when written, else C), by one atomic
                                                          per wave (order-independent, deterministic); the caller
                                                          zeroes it first.  The |D| / |A| bound of the fp16-pair
                                                          weight gradient (ot_mixed_gemm_wgrad_ex) */
  float* rowabs_out; int rowabs_n;                     /* optional, whole-tile kernels: each 128-column tile's max
                                                          |v| of every output row (v as for amax_out) at
                                                          [out_row][tile], rowabs_n = ceil(N / 128): the row bounds
                                                          (a_rowmax) of an fp16-pair consumer GEMM whose A this is */
} ot_rms_epilogue;
size_t ot_mixed_gemm_rms_workspace_size(int ntiles, int N);
int ot_mixed_gemm_rms(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                      int a_xform, const float* a_rstd, const float* a_gamma,
                      const float* W, int64_t w_gstride, int64_t ldw, int N,
                      const int32_t* tile_group, int ntiles,
                      const float* bias, int64_t bias_gstride,
                      float* C, int64_t ldc, const int32_t* out_rows, int epi,
                      const float* res, int64_t ldres, int res_tok,
                      const float* aux, int64_t ldaux,
                      uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                      const int32_t* tail_pos, const ot_rms_epilogue* rms, int precision, void* stream);

/* dW[g] (+)= sum pro(A[a_rows])^T D[d_rows], db[g] (+)= sum D[d_rows] over the rows of every
 * chunk of group g.  chunks: [nchunks][3] {group, row_begin, row_count} indexing the row maps;
 * gchunk: [ngroups][2] {first chunk, chunk count} (a group's chunks are contiguous).
 * Deterministic: per-chunk partial slabs summed in chunk order. */
size_t ot_wgrad_workspace_size(int nchunks, int K, int N);
int ot_mixed_gemm_wgrad(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                        const float* a_rstd, const float* a_gamma,
                        const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                        const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                        float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                        int accumulate, void* workspace, size_t ws_bytes, int precision, void* stream);

/* ot_mixed_gemm_wgrad on the scaled fp16 pair (OT_MATMUL_SPLIT_BF16, f32 operands, a_xform OT_AX_NONE /
 * OT_AX_RMSNORM / OT_AX_GELU): A column k and D are scaled by powers of two from magnitude bounds and split into an
 * fp16 pair (x s = h + l, 22 significant bits of each element down to 2^-16 of its bound), three f16 products per
 * f32 product instead of the six bf16 ones.  d_bound: one float >= max |D| over the rows used; a_bound: one float
 * >= max |A'| of the transformed A (GELU: >= max |A|, since |gelu(u)| <= |u|), not needed with OT_AX_RMSNORM
 * (|x_k rstd gamma_k| <= sqrt(K) |gamma_k|).  The bounds are device pointers, typically the amax outputs of the
 * operands' producers (ot_rms_epilogue.amax_out, ot_dropout_apply_ex, ot_attn_fwd_amax, ot_attn_bwd_amax).
 * With d_bound NULL (or a_bound NULL where needed, or another mode / form) the call is ot_mixed_gemm_wgrad. */
int ot_mixed_gemm_wgrad_ex(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                           const float* a_rstd, const float* a_gamma,
                           const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                           const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                           float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                           int accumulate, void* workspace, size_t ws_bytes, const float* a_bound,
                           const float* d_bound, int precision, void* stream);

/* ot_mixed_gemm_wgrad_ex's pair form with the GELU prologue (a_xform OT_AX_GELU | OT_WG_D_KEEPBITS, split mode,
 * N % 128 == 0) on D' = keep ? D * d_scale : 0: D holds the gradient before a dropout mask, keep [d_row][ldkeep]
 * uint32 the rows' keep bits in column order (bit n % 32 of word n / 32; ot_ffn_fused_bwd_mask's keep_out), d_scale
 * 1 / (1 - rate).  d_bound: >= max |D|, before the mask (the kernel multiplies it by d_scale).  dW and db equal the
 * call on a materialised D' whose d_bound has the scale of d_bound * d_scale, bit for bit.  ldkeep % 4 == 0, keep
 * 16-B aligned. */
int ot_mixed_gemm_wgrad_keep(const float* A, int64_t lda, const int32_t* a_rows, int a_xform,
                             const float* D, int64_t ldd, const int32_t* d_rows, int K, int N,
                             const int32_t* chunks, int nchunks, const int32_t* gchunk, int ngroups,
                             float* dW, int64_t dw_gstride, float* db, int64_t db_gstride,
                             int accumulate, void* workspace, size_t ws_bytes, const float* a_bound,
                             const float* d_bound, const uint32_t* keep, int64_t ldkeep, float d_scale,
                             int precision, void* stream);

/* Transposed weight shadow for the forward GEMMs (NT staging reads k-contiguous rows):
 * dst[g][n][k] = src[g][k][n] per bank; banks_dev: [nbanks][6] int64 {src_off, dst_off, G, K, N,
 * first_tile}, a bank owning G*ceil(K/32)*ceil(N/32) consecutive 32x32 tiles of the launch. */
int ot_transpose_banks(const float* src, float* dst, const int64_t* banks_dev, int nbanks, int64_t total_tiles,
                       void* stream);

/* Pre-split B images for the plane GEMM (split-bf16 mode).  A weight bank used as the B operand
 * B[g][n][k] = src[g*gstride + n*sn + k*sk] (* kscale[k] when kscale_off >= 0: an RMSNorm gamma folded
 * into the weights, x*rstd*gamma @ W = rstd * (x @ (gamma W))) is written once per weight update as
 * its three exact bf16 planes, one 12-KiB block per (g, 128-column tile, 16-k stage) in the LDS image
 * the GEMM reads — except a gamma-folded bank (the RMSNorm-prologue GEMMs'), written as the scaled fp16
 * pair of B[g][n][k] s_n (s_n a power of two per column n putting its largest magnitude in [2^13, 2^14),
 * stored as 128 floats in the third plane of the tile's first block), which those GEMMs multiply with three
 * f16 products (A scaled per row from the bound |x| <= sqrt(K) / rstd).  desc_dev: [ndesc][10] int64 {src_off, sn, sk, gstride, kscale_off, dst_off
 * (elements of img), first_unit, G, N, K} (offsets into base; K % 16 == 0; kscale_off -1: none, -2: none
 * and the pair form — the FFN2 forward's W2 image, read with ot_rms_epilogue.a_rowmax); a bank owns
 * G*ceil(N/128)*(K/16) consecutive units of the launch; ot_split_image_elems gives its size. */
size_t ot_split_image_elems(int G, int N, int K);
int ot_split_images(const float* base, const int64_t* desc_dev, int ndesc, int64_t total_units, uint16_t* img,
                    int precision, void* stream);
/* How ot_split_images builds: 1 (default) = one launch, one workgroup per (bank, g, 128-column tile) that takes the
 * tile's column maxima and then splits its K / 16 units; 0 = the two launches with one workgroup per unit (column
 * scales, then the split), kept as the reference of tests/test_image_build_gpu.py.  Same image bytes either way.  The
 * environment variable ONETRANS_IMAGE_BUILD (0 / 1) sets the process's initial value.  Process-wide; on = -1 only
 * queries; returns the previous setting. */
int ot_image_build(int on);
/* ot_mixed_gemm / ot_mixed_gemm_rms with the B operand's pre-split image (b_image: the bank's image,
 * image_ntn column tiles per group, the GEMM's columns starting at tile image_tn0).  In split mode,
 * NT, whole tiles and 16-B aligned A rows the plane GEMM runs (B by global_load_lds from the image,
 * A split once per tile at fragment time); with a_xform = OT_AX_RMSNORM the image must carry gamma
 * (kscale) and only a_rstd is read.  Otherwise the call is ot_mixed_gemm / ot_mixed_gemm_rms. */
int ot_mixed_gemm_img(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                      int a_xform, const float* a_rstd, const float* a_gamma,
                      const float* W, int64_t w_gstride, int64_t ldw, int N,
                      const int32_t* tile_group, int ntiles,
                      const float* bias, int64_t bias_gstride,
                      float* C, int64_t ldc, const int32_t* out_rows, int epi,
                      const float* res, int64_t ldres, int res_tok,
                      const float* aux, int64_t ldaux,
                      uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                      const int32_t* tail_pos, const uint16_t* b_image, int image_ntn, int image_tn0,
                      int precision, void* stream);
/* The bf16-mode plane GEMM's tile for N % 256 == 0, K % 32 == 0: 0 = 128 x 128, 1 = auto (default: 128 x 256 when
 * N <= K, else 128 x 128), 2 / 3 / 4 = 128 x 256 / 128 x 512 / 256 x 256 where the shape allows; every tile gives
 * the same outputs bit for bit (fewer L2 -> LDS bytes per MFMA on the larger ones).  Process-wide; on = -1 only
 * queries; returns the previous setting.  A tuning and test knob. */
int ot_plane_wide(int on);
/* The bf16 weight gradient's (OT_WG_D_BF16 with OT_AX_BF16 A) tile: 0 = 128 x 128, 1 = auto (default: 256 x 256
 * where K % 256 == N % 256 == 0, else 128 x 256 where N % 256 == 0), 2 = 128 x 256, 3 = 256 x 256; the same slabs
 * bit for bit.  Same switch semantics as ot_plane_wide. */
int ot_wgrad_wide(int on);
/* The split-mode pair plane GEMM's epilogue row metadata (output rows, RMSNorm row factors): 1 = loaded once per
 * tile and parked in LDS (default), 0 = read from the row maps per epilogue row batch.  The same values, so the
 * same outputs bit for bit.  Process-wide; on = -1 only queries; returns the previous setting. */
int ot_plane_rowmeta(int on);
/* The panel form of the split-mode pair plane GEMM (one workgroup walks a row tile's column tiles and copies the
 * next tile's first stages during the epilogue): 0 = off (default: every launch on the one-tile kernel; the panel
 * form measured no faster), 1 = auto (pair launches with N >= 256 under the RMSNorm prologue with epilogue 0 /
 * OT_EPI_BIAS, or plain A with a_rowmax and OT_EPI_GELU_BWD [| OT_EPI_ROWDOT]; launches too small to fill the
 * device stay on the one-tile kernel), w in 2 .. 64 = on with w column tiles per workgroup, 100 + w = the same on
 * the four-workgroups-per-CU variant, 200 + w = on the variant that holds A's fragments across the column tiles
 * (K = 128 only).  Bit-identical outputs.  Process-wide; on = -1 only queries; returns the previous setting. */
int ot_plane_panel(int on);
/* Number of GEMM launches that took the panel form since the library was loaded, modulo 2^31 (tests: which kernel
 * ran). */
int ot_plane_panel_launches(void);
int ot_mixed_gemm_rms_img(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                          int a_xform, const float* a_rstd, const float* a_gamma,
                          const float* W, int64_t w_gstride, int64_t ldw, int N,
                          const int32_t* tile_group, int ntiles,
                          const float* bias, int64_t bias_gstride,
                          float* C, int64_t ldc, const int32_t* out_rows, int epi,
                          const float* res, int64_t ldres, int res_tok,
                          const float* aux, int64_t ldaux,
                          uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                          const int32_t* tail_pos, const ot_rms_epilogue* rms, const uint16_t* b_image,
                          int image_ntn, int image_tn0, int precision, void* stream);

/* The fused FFN forward of the split mode at hidden width 128 (model.py:154-161, 198):
 *   u = rstd * (x1 @ (gamma W1[g])) + b1[g],  x2 = x1 + drop(gelu(u) @ W2[g] + b2[g])  [, rstd_out = rstd(x2)]
 * in one launch: a row tile's u stays in the accumulators between the two products (scaled fp16 pair arithmetic, as
 * the OT_AX_RMSNORM / OT_AX_GELU plane GEMMs with pair-form images), so u is neither read back nor, without u_out,
 * written.  u (when written) equals the FFN1 launch's bit for bit; x2 differs from the FFN2 launch's by rounding (a
 * row scale per 128 columns of u instead of one per row, another k order).  The dropout mask, bias, residual and
 * rstd arithmetic are the FFN2 epilogue's. */
typedef struct ot_ffn_fused_args {
  size_t struct_size;                                  /* sizeof(ot_ffn_fused_args): any other value is refused */
  const float* x1; int64_t ldx1;                       /* FFN input and residual rows, 128 floats each */
  const int32_t* rows;                                 /* [ntiles * 128] row of x1 / u / x2 per tile row, -1 = none;
                                                          NULL = identity */
  const int32_t* tile_group; int ntiles;               /* weight group per tile (NULL: group 0) */
  const float* rstd;                                   /* norm2's rstd per x1 row */
  const uint16_t* w1_image; int w1_groups;             /* ot_split_images pair images: W1 forward (gamma folded, f / 128 */
  const uint16_t* w2_image; int w2_groups;             /* column tiles of 8 units per group), W2 forward (f / 16 units) */
  const float* b1; int64_t b1_gstride;
  const float* b2; int64_t b2_gstride;
  int f;                                               /* FFN width: a multiple of 128, at most 1024 */
  float* u_out; int64_t ldu;                           /* optional (training): u */
  float* u_amax;                                       /* optional: *u_amax = max(*u_amax, max |u|) as amax_out */
  float* x2; int64_t ldx2;
  float* rstd_out; float eps;                          /* optional: the next RMSNorm's rstd (OT_EPI_ROW_RSTD) */
  uint32_t seed, site; float drop_rate;                /* dropout as ot_mixed_gemm's (0: none) */
  int tail_K, tail_I; const int32_t* tail_pos;
} ot_ffn_fused_args;
int ot_ffn_fused_fwd(const ot_ffn_fused_args* args, void* stream);
/* Whether the model's block forward takes ot_ffn_fused_fwd where its form applies (1, default) or the FFN1 and FFN2
 * launches (0).  Process-wide; on = -1 only queries; returns the previous setting.  The library only keeps the
 * setting: the host layer reads it. */
int ot_ffn_fused(int on);

/* The fused FFN backward of the split mode at hidden width 128: the two input gradients of the FFN branch
 *   dU = (dy2 @ W2[g]^T) * gelu'(u),  dx1 = norm2_bwd(dU @ W1[g]^T; x1, rstd, gamma) + dres  [, dx_masked = drop(dx1)]
 * in one launch: a row tile's dU is written once (the W1 weight gradient and db1 read it) and multiplied from the
 * accumulators, so it is not read back and its row maxima never pass through memory.  dU and *du_amax equal the FFN2
 * dgrad launch's (ot_mixed_gemm_rms_img, OT_EPI_GELU_BWD, a_rowmax = dy2_rowmax) bit for bit; dx1 / dx_masked / dgamma
 * differ from the FFN1 dgrad launch's (OT_EPI_RMSNORM_BWD [| OT_EPI_DROPOUT]) by rounding (a row scale per 128 columns
 * of dU — the largest |dU| of the row's columns so far — instead of one per row, another k order).  The norm backward,
 * dropout mask, dgamma, amax_out and rowabs_out arithmetic are that epilogue's. */
typedef struct ot_ffn_fused_bwd_args {
  size_t struct_size;                                  /* sizeof(ot_ffn_fused_bwd_args): any other value is refused */
  const float* dy2; int64_t lddy2;                     /* gradient of the FFN branch's output, 128 floats per row */
  const float* dy2_rowmax; int dy2_rowmax_n;           /* [dy2 row][n] parts of max |dy2| per row (a_rowmax) */
  const int32_t* rows;                                 /* [ntiles * 128] row of dy2 / u / du / x1 / dx1 per tile row,
                                                          -1 = none; NULL = identity */
  const int32_t* tile_group; int ntiles;               /* weight group per tile (NULL: group 0) */
  const uint16_t* w2_image; int w2_groups;             /* ot_split_images pair images of the dgrads: W2 (f / 128 column */
  const uint16_t* w1_image; int w1_groups;             /* tiles of 8 units per group), W1 (f / 16 units per group) */
  int f;                                               /* FFN width: a multiple of 128, at most 1024 */
  const float* u; int64_t ldu;                         /* the forward's pre-activation */
  float* du; int64_t lddu;
  float* du_amax;                                      /* optional: *du_amax = max(*du_amax, max |du|) as amax_out */
  const float* x1; int64_t ldx1;                       /* norm2's input, gamma and rstd */
  const float* gamma; const float* rstd;
  const float* dres; int64_t lddres;                   /* optional: added to dx1 (the residual branch's gradient) */
  float* dx1; int64_t lddx1;
  float* dx_masked; int64_t lddxm;                     /* with drop_rate > 0: drop(dx1) at (seed, site) */
  float* dgamma; int accumulate_dgamma;
  void* workspace; size_t ws_bytes;                    /* ot_mixed_gemm_rms_workspace_size(ntiles, 128) */
  float* amax_out; float* rowabs_out; int rowabs_n;    /* optional, as ot_rms_epilogue's (of dx_masked, else dx1); rowabs_n 1 */
  uint32_t seed, site; float drop_rate;                /* dropout as ot_mixed_gemm's (0: none) */
  int tail_K, tail_I; const int32_t* tail_pos;
} ot_ffn_fused_bwd_args;
int ot_ffn_fused_bwd(const ot_ffn_fused_bwd_args* args, void* stream);
/* Whether the model's block backward takes ot_ffn_fused_bwd where its form applies (1, default) or the FFN2 and FFN1
 * dgrad launches (0); the environment variable ONETRANS_FFN_FUSED_BWD (0 / 1) sets the process's initial value.
 * Process-wide; on = -1 only queries; returns the previous setting.  The library only keeps the setting: the host
 * layer reads it. */
int ot_ffn_fused_bwd_on(int on);
/* ot_ffn_fused_bwd with the FFN dropout's backward inside it (drop_rate > 0): args->dy2 is dx2, the gradient before
 * the mask, and args->dy2_rowmax bounds |dx2| per row (the kernel multiplies the bound by 1 / (1 - drop_rate)).  The
 * kernel forms dy2 = keep ? dx2 / (1 - drop_rate) : 0 at fragment time, the mask that ot_dropout_apply_ex(dx2, seed,
 * mask_site, drop_rate, tail map) applies, with the same f32 multiply: given row bounds with the scale of that pass's
 * row maxima, every output equals {ot_dropout_apply_ex, ot_ffn_fused_bwd on its dy2} bit for bit.  (args->site stays
 * the site of dx_masked.)  keep_out: [row][ldkeep] uint32, the row's 128 keep bits in column order (bit c % 32 of
 * word c / 32), written for the rows the map names: the D mask of the W2 weight gradient (ot_mixed_gemm_wgrad_keep).
 * ldkeep % 4 == 0, keep_out 16-B aligned. */
int ot_ffn_fused_bwd_mask(const ot_ffn_fused_bwd_args* args, uint32_t mask_site, uint32_t* keep_out, int64_t ldkeep,
                          void* stream);
/* Whether the model's block backward, where it takes ot_ffn_fused_bwd under dropout, masks dx2 inside that kernel and
 * inside the W2 weight gradient (1, default: no dropout pass, no dy2) or runs the dropout pass first (0); the
 * environment variable ONETRANS_BWD_MASK_FUSED (0 / 1) sets the process's initial value.  Process-wide; on = -1 only queries;
 * returns the previous setting.  The library only keeps the setting: the host layer reads it. */
int ot_bwd_mask_fused(int on);

/* ---- causal attention with a query tail (attention.hip; kernels: attn.h lists the files) --
 * Replaces model.py:100-114 (einsum QK^T/sqrt(hd), band_part mask with -1e9, softmax, einsum PV)
 * and the pyramid gather of queries model.py:356/371 (only the last K of I queries computed).
 * qkv: [B*I, ld] (q | k | v, head h at +h*head_dim); out: [B*K, H*head_dim]; lse: [B, H, K].
 * qpos: NULL (query j of a sample sits at position I - K + j) or the ascending kept positions
 * [B*K] of ot_pyramid_select (query j at qpos[b*K + j], causal limit key <= qpos). */
int ot_attn_fwd(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                int head_dim, float* out, float* lse, int precision, void* stream);
/* The same forward on block-scaled fp8 MFMA (attention_fp8.hip; BASELINE configs[4] "CDNA4 fp8 MFMA
 * attention"): K and Q quantised to OCP e4m3 with one e8m0 scale per (row, 32 dims), V with one scale
 * per (dim, 64 keys), P = exp(s - m) as e4m3 of P * 2^8; v_mfma_scale_f32_32x32x64_f8f6f4 for QK^T and
 * PV, softmax statistics and O accumulation in f32.  head_dim 64 or 128.  Reduced precision (not the
 * reference's f32): out / lse as ot_attn_fwd within the fp8 bounds of tests/test_attn_fp8_gpu.py.
 * workspace: ot_attn_fwd_fp8_workspace_size(B, H, I, head_dim) bytes, 16-B aligned (the packed
 * fp8 K / V^T images and their scales). */
size_t ot_attn_fwd_fp8_workspace_size(int B, int H, int I, int head_dim);
int ot_attn_fwd_fp8(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                    int head_dim, float* out, float* lse, void* workspace, size_t ws_bytes, void* stream);
/* flags of ot_attn_fwd_fp8_ex */
#define OT_FP8_DEQUANT 1 /* training: overwrite qkv's Q (kept query rows), K and V with their dequantised fp8
                          * values, so ot_attn_bwd in the bf16 GEMM mode recomputes S from (nearly) the operands
                          * the fp8 forward used.  One term (e4m3 x block scale) is exact in bf16 and the
                          * backward's P then matches this lse up to summation order.  With OT_FP8_TWO_TERM the
                          * dequantised value hi + lo has more than bf16's 8 significant bits (the bf16 backward
                          * rounds it) and the forward dropped the lo.lo product, so the recomputed S differs from
                          * the forward's by those two terms: the straight-through gradient is approximate
                          * (tests/test_attn_fp8_gpu.py: 0.5-1% of max|g| from the exact attention gradient) */
#define OT_FP8_TWO_TERM 2 /* two-term e4m3 operands: every Q / K / V / P element as hi = e4m3(x) plus lo =
                           * e4m3(x - hi), each with its own block scale; QK^T and PV as three fp8 MFMA
                           * products (hi.hi + hi.lo + lo.hi): ~7 significant bits per operand */
int ot_attn_fwd_fp8_ex(float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos, int head_dim,
                       float* out, float* lse, void* workspace, size_t ws_bytes, int flags, void* stream);
/* ot_attn_fwd_fp8_ex with OT_FP8_DEQUANT implied and the dequantised Q (kept rows) / K / V written rounded to
 * bf16 into deq16 ([B*I][ld] uint16, the qkv layout; 16-B aligned, ld % 8 == 0) instead of in place: the
 * bf16 backward's operands (OT_ATTN_QKV_BF16), which it would round so anyway; qkv is only read */
int ot_attn_fwd_fp8_deq16(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                          int head_dim, float* out, float* lse, void* workspace, size_t ws_bytes, int flags,
                          uint16_t* deq16, void* stream);
/* dqkv: like qkv (dq written on the K kept query rows only; dk, dv on all rows);
 * ws: ot_attn_bwd_workspace_size(B, H, K) bytes (row stats padded to 32 queries per (b, h)) */
size_t ot_attn_bwd_workspace_size(int B, int H, int K);
int ot_attn_bwd(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv, float* delta_ws,
                int precision, void* stream);
/* ot_attn_bwd with a sized workspace: given ot_attn_bwd_ex_workspace_size(B, H, I, K, head_dim,
 * qpos != NULL, precision) bytes, the bf16-mode backward splits each (sample, head)'s key blocks over several
 * waves when B*H alone cannot fill the chip (C5: 4 slices), their dQ partials summed in a fixed
 * order (deterministic); with ot_attn_bwd_workspace_size bytes it runs as ot_attn_bwd. */
size_t ot_attn_bwd_ex_workspace_size(int B, int H, int I, int K, int head_dim, int selected, int precision);
int ot_attn_bwd_ex(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                   int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv, void* workspace,
                   size_t ws_bytes, int precision, void* stream);
/* ot_attn_bwd_ex with output flags.  OT_ATTN_DQKV_BF16: dqkv holds bf16 (uint16 bits, ld in elements,
 * 8-B aligned) — the bf16 mode's consumers (the QKV dgrad's A operand, the Wqkv weight gradient's D) round
 * it to bf16 anyway, so the values they use are unchanged (each element is the f32 result rounded once).
 * Key-grouped backward only (ot_attn_bwd_dqkv_bf16_supported); workspace
 * ot_attn_bwd_flags_workspace_size (one more [B*K][H*head_dim] f32 dQ slot: slice 0's). */
#define OT_ATTN_DQKV_BF16 1
/* OT_ATTN_QKV_BF16: qkv holds bf16 (uint16 bits, ld in elements, 16-B aligned): the fp8 forward's dequantised
 * operands from ot_attn_fwd_fp8_deq16 (same key-grouped condition) */
#define OT_ATTN_QKV_BF16 2
/* OT_ATTN_DQ_PART_BF16 (with OT_ATTN_DQKV_BF16): the key slices' dQ partials are kept in bf16 (summed in f32,
 * then rounded: not the f32 sum rounded once — about one more bf16 rounding of each partial) */
#define OT_ATTN_DQ_PART_BF16 4
int ot_attn_bwd_dqkv_bf16_supported(int I, int K, int head_dim, int selected, int precision);
/* the OT_ATTN_*_BF16 flags the backward supports at this shape: all three on the key-grouped bf16 backward,
 * OT_ATTN_DQKV_BF16 alone on the short-tail kernel (K <= 4: the last layer after DCE), none otherwise */
int ot_attn_bwd_bf16_forms(int I, int K, int head_dim, int selected, int precision);
/* (in the f32-accurate mode it also covers the head_dim-64 slice backward's dS scratch: one causal block pair
 * store per co-resident workgroup, two per CU — one per CU for the long form, K <= 272 / I <= 544; a smaller
 * workspace shrinks that kernel's grid, and below one workgroup's share per CU the long forms (I > 144) are not
 * taken: the per-pair f32 backward runs instead) */
size_t ot_attn_bwd_flags_workspace_size(int B, int H, int I, int K, int head_dim, int selected, int flags, int precision);
/* 1 when the f32-accurate mode (OT_MATMUL_SPLIT_BF16) runs this shape's forward and backward as one
 * workgroup per (sample, head) slice on split MFMA (attention_slice.hip: head_dim 32 / 64, I <= 192,
 * tail queries for the backward, the slice's planes within LDS; the dS store in LDS at head_dim 32, in the
 * workspace at 64), else 0.  (The backward alone also takes head_dim 64 up to I 544 / K 272 on the slice
 * kernels, with a forward from attn_fwd_split_kernel: ot_attn_bwd_flags_workspace_size then exceeds
 * ot_attn_bwd_workspace_size by its dS scratch.) */
int ot_attn_slice_supported(int I, int K, int head_dim, int selected);
int ot_attn_bwd_flags(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                      int B, int H, int I, int K, const int32_t* qpos, int head_dim, void* dqkv, int flags,
                      void* workspace, size_t ws_bytes, int precision, void* stream);
/* Output bounds for the fp16-pair weight gradients (ot_mixed_gemm_wgrad_ex): ot_attn_fwd / ot_attn_bwd_ex that also
 * fold max |O| (forward) or max |dQKV| (backward) into *amax (one float the caller zeroes; atomic max, deterministic).
 * Only where the slice kernels run the shape — ot_attn_amax_supported: bit 1 the forward (OT_MATMUL_SPLIT_BF16, K > 4,
 * the slice forward's shapes), bit 2 the backward (also qpos NULL, the slice backward's shapes; it needs
 * ot_attn_bwd_flags_workspace_size bytes) — elsewhere the call is refused. */
int ot_attn_amax_supported(int I, int K, int head_dim, int selected, int precision);
/* rowmax (optional, either may be NULL): per-row maxima of |output| for an fp16-pair dgrad consumer's a_rowmax —
 * forward [B*K][H] (row b*K + j, head h: max |O| over the head's columns), backward [B*I][3][H] (row b*I + p: the dQ,
 * dK, dV parts per head; with K < I the dQ part of the rows without a query is not written: zero the array first) */
int ot_attn_fwd_amax(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos,
                     int head_dim, float* out, float* lse, float* amax, float* rowmax, int precision, void* stream);
int ot_attn_bwd_amax(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse,
                     int B, int H, int I, int K, const int32_t* qpos, int head_dim, float* dqkv,
                     void* workspace, size_t ws_bytes, float* amax, float* rowmax, int precision, void* stream);

/* Two-stage cached serving (paper §3.5.1; replaces the reference's defective cache path
 * model.py:94-98, 359-381, D6): candidate c (request req[c]) attends with the last Kq of its n
 * N-side rows (qkv [C*n, ld], q | k | v) over its request's Ic cached S-side rows (kv_cache
 * [R*Ic, ldc], k at col 0, v at col d) and its own n rows, causally (query j at absolute position
 * Ic + n - Kq + j).  out: [C*Kq, H*head_dim].  Forward only. */
int ot_attn_fwd_cached(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc, const int32_t* req,
                       int C, int H, int Ic, int n, int Kq, int head_dim, float* out, void* stream);

/* Request-grouped training: the cached attention with a backward.  ot_attn_fwd_cached_lse is
 * ot_attn_fwd_cached (same out, bit for bit) that also writes lse [C, H, Kq] in ot_attn_fwd's convention
 * (natural log of the softmax denominator of the whole row: cached keys and own rows).
 * ot_attn_bwd_cached: req_start [R+1] gives request r's candidates [req_start[r], req_start[r+1]) (candidates
 * sorted by request).  dqkv [C*n, ld]: dq on the Kq kept rows of each candidate only (the other rows' q columns
 * are not written), dk | dv on all n rows.  dkv_cache [R*Ic, ldc] (dK at col 0, dV at col d): the sum over the
 * request's candidates in candidate order, one writer per element (no atomics; bit-identical from run to run);
 * accumulate 0 writes it (zeros for a request without candidates), 1 adds to what is there.  Native f32 MFMA.
 * workspace: ot_attn_bwd_cached_workspace_size bytes. */
int ot_attn_fwd_cached_lse(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc, const int32_t* req,
                           int C, int H, int Ic, int n, int Kq, int head_dim, float* out, float* lse, void* stream);
size_t ot_attn_bwd_cached_workspace_size(int R, int C, int H, int Ic, int n, int Kq, int head_dim);
int ot_attn_bwd_cached(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc, const int32_t* req_start,
                       int R, int C, int H, int Ic, int n, int Kq, int head_dim, const float* out, const float* dout,
                       const float* lse, float* dqkv, float* dkv_cache, int accumulate, void* workspace,
                       size_t ws_bytes, void* stream);

/* ---- one-query attention folded through the shared K / V projection (attention_fold.hip) -----
 * The last layer keeps one query per sample (K = 1, the last position, which sees every key).  For the keys of
 * weight group 0 the projection K_j = Wk0^T (gamma o xh_j), xh_j = x_j rstd_j, need not be formed: head h's score is
 * <xh_j, gamma o (Wk0[:, h] q_h)> / sqrt(hd) and its value sum Wv0[:, h]^T (gamma o y_h), y_h = sum_j p_h[j] xh_j.
 * The keys at positions ded0 <= p < ded1 (the dedicated groups) keep their projected rows.
 *   x [B*I, ldx], rstd [B*I], gamma [d]: the layer input, its RMSNorm rstd and norm1's weight
 *   w [d][ldw >= 3d]: group 0's Wqkv (Wk at column d, Wv at 2d); wT [3d][ldwT >= d]: its transpose
 *   qkv [B*I, ldqkv]: q in columns 0..d of each sample's last row, K | V in columns d..3d of the dedicated rows
 *   o [B, d], lse [B, H] (natural log, ot_attn_fwd's layout at K = 1), y [B, H, d]
 * ot_attn_fold_supported: d = 128 with 2 or 4 heads (anything else: OT_ERR_UNSUPPORTED; the caller runs ot_attn_fwd).
 * ot_attn_fold_bwd, given dout [B, d] and the forward's o / lse / y, writes
 *   dx [B*I, lddx]: for a group-0 row the gradient through its use as a key, norm1's backward applied; zero for a
 *     dedicated row; the query row also gets dx1[b] (optional, [B, d]: the residual branch) added
 *   dqkv [B*nf, lddqkv >= 3d], nf = ot_attn_fold_rows(I, ded0, ded1): row b*nf + (p - ded0) of dedicated position p
 *     holds 0 | dK | dV; the query's row (that row when it is dedicated, else b*nf + ded1 - ded0) holds dq in columns
 *     0..d (and 0 in d..3d when it is not dedicated)
 *   z [B, H, d]: z_h = sum_j ds_h[j] xh_j;  dgpart [B, d]: each sample's part of norm1's dgamma
 * ot_attn_fold_dw: dW[k][d + n] (+)= gamma[k] sum_b z[b][head(n)][k] q[b][n] and dW[k][2d + n] (+)= gamma[k] sum_b
 * y[b][head(n)][k] dout[b][n] (dW: group 0's Wqkv gradient [d][lddw >= 3d]); ot_attn_fold_dgamma: dgamma (+)= sum_b
 * dgpart[b].  Both sum per-chunk partials in a fixed order (no float atomics); workspace: ot_attn_fold_workspace_size.
 * ot_last_fold: whether the model's last block takes this path where its gate holds (1, default; environment
 * variable ONETRANS_LAST_FOLD) or the ot_attn_fwd launches (0).  Process-wide; on = -1 only queries; returns the
 * previous setting.  The library only keeps the setting: the host layer reads it. */
int ot_attn_fold_supported(int d, int H);
int ot_attn_fold_rows(int I, int ded0, int ded1);
int ot_attn_fold_fwd(const float* x, int64_t ldx, const float* rstd, const float* gamma, const float* w, int64_t ldw,
                     const float* wT, int64_t ldwT, const float* qkv, int64_t ldqkv, int B, int H, int I,
                     int head_dim, int ded0, int ded1, float* o, float* lse, float* y, void* stream);
int ot_attn_fold_bwd(const float* x, int64_t ldx, const float* rstd, const float* gamma, const float* w, int64_t ldw,
                     const float* wT, int64_t ldwT, const float* qkv, int64_t ldqkv, int B, int H, int I,
                     int head_dim, int ded0, int ded1, const float* o, const float* dout, const float* lse,
                     const float* y, const float* dx1, float* dx, int64_t lddx, float* dqkv, int64_t lddqkv, float* z,
                     float* dgpart, void* stream);
size_t ot_attn_fold_workspace_size(int B, int d);
int ot_attn_fold_dw(const float* z, const float* y, const float* qkv, int64_t ldqkv, const float* dout,
                    const float* gamma, int B, int H, int I, int head_dim, float* dW, int64_t lddw, int accumulate,
                    void* workspace, size_t ws_bytes, void* stream);
int ot_attn_fold_dgamma(const float* dgpart, int B, int d, float* dgamma, int accumulate, void* workspace,
                        size_t ws_bytes, void* stream);
int ot_last_fold(int on);

/* ---- padding mask (attention.hip, seqfuse.hip) ---------------------------------------------
 * Variable-length histories: behaviour sequences arrive left-padded to their cap, and with a key-padding mask a
 * padding event is no key for any other token.  key_valid is a byte per (sample, key): key_valid[b * ldv + j] != 0
 * when key j of sample b is a real token (ldv >= I; a layer of I tokens under the tail keep reads layer 0's array
 * through a pointer offset L0 - I with ldv = L0).  Query at position i sees key j iff j <= i and (valid j or
 * j == i): the self exception gives every row one visible key (no empty softmax), and since a valid row never sees
 * an invalid key, a padding row's content reaches no valid row in any layer.  A padding query's output is its own v.
 *
 * ot_attn_fwd_masked / ot_attn_bwd_masked: ot_attn_fwd / ot_attn_bwd with that rule (same operands, outputs, lse
 * convention and ot_attn_bwd_workspace_size workspace).  They run the generic f32 family at every shape for
 * OT_MATMUL_F32 and OT_MATMUL_SPLIT_BF16 (short-tail kernels at K <= 4, else the f32 MFMA forward and the prep +
 * f32 MFMA backward; results do not depend on which of the two precisions is named); OT_MATMUL_BF16 returns
 * OT_ERR_UNSUPPORTED.  No magnitude bounds are reported.
 * ot_attn_fwd_cached_masked: ot_attn_fwd_cached / ot_attn_fwd_cached_lse (lse_or_null) with cache_valid
 * [R][ldcv >= Ic] bytes over the cached rows; a candidate's own n rows are always valid.
 *
 * ot_seq_key_valid writes layer 0's array valid0 [B][L0] in one stream-ordered launch (no host sync).  lens: device
 * int32 [nseq][B], the number of real events of each present sequence (the last lens of its seq_len[i] positions;
 * values outside [0, seq_len[i]] are clamped on the device).  seq_len / seq_off: HOST arrays [nseq], each sequence's
 * cap and the token position of its first event (ascending, disjoint).  Every token outside the segments ([SEP], NS)
 * is valid.  rank NULL: event j of sequence i sits at seq_off[i] + j.  rank given (time fusion: ot_seq_time_rows'
 * rank_out, row stride ldr): it sits at rank[b * ldr + start_i + j], start_i = seq_len[0] + .. + seq_len[i-1]; the
 * segments must then be the positions 0 .. sum(seq_len) - 1 without gaps.  nseq <= 32. */
int ot_attn_fwd_masked(const float* qkv, int64_t ld, int B, int H, int I, int K, const int32_t* qpos, int head_dim,
                       const uint8_t* key_valid, int64_t ldv, float* out, float* lse, int precision, void* stream);
int ot_attn_bwd_masked(const float* qkv, int64_t ld, const float* out, const float* dout, const float* lse, int B,
                       int H, int I, int K, const int32_t* qpos, int head_dim, const uint8_t* key_valid, int64_t ldv,
                       float* dqkv, float* delta_ws, int precision, void* stream);
int ot_attn_fwd_cached_masked(const float* qkv, int64_t ld, const float* kv_cache, int64_t ldc, const int32_t* req,
                              int C, int H, int Ic, int n, int Kq, int head_dim, const uint8_t* cache_valid,
                              int64_t ldcv, float* out, float* lse_or_null, void* stream);
int ot_seq_key_valid(const int32_t* lens, const int32_t* seq_len, const int32_t* seq_off, int nseq, int B, int L0,
                     const int32_t* rank, int64_t ldr, uint8_t* valid0, void* stream);

/* ---- bf16 request cache for serving (attention_kv16.hip) -----------------------------------
 * The cached S-side K/V rows of a request, stored rounded to bf16 (round to nearest even, NaN stays NaN, a value
 * past the bf16 range becomes +-inf) in rows of ldc16 elements (ldc16 % 8 == 0, >= 2d: K at col 0, V at col d),
 * request r owning rows [r*req_stride, (r+1)*req_stride).  Rounding happens only when a row is stored; the
 * attention widens the rows in registers and computes in f32, a candidate's own rows stay f32.
 *
 * ot_kv_pack_bf16: K | V columns [d, 3d) of qkv row r*rows_per_req + i -> row r*req_stride + row0 + i, cols
 * [0, 2d) of kv16 (r < R, i < rows_per_req; d % 4 == 0, req_stride >= row0 + rows_per_req).  One pass, 16-byte
 * loads and stores; columns >= 2d and rows outside [row0, row0 + rows_per_req) of each request are not written.
 * ot_attn_fwd_cached_kv16: ot_attn_fwd_cached_masked over such a cache: request r's key j (j < Ic <= req_stride) is
 * kv16 row r*req_stride + j.  cache_valid NULL = every cached row valid.  Same out / lse convention.
 * qkv, kv16 and out are 16-byte aligned.  R == 0 / C == 0 return OT_OK without a launch. */
int ot_kv_pack_bf16(const float* qkv, int64_t ld, int R, int64_t rows_per_req, int d, uint16_t* kv16, int64_t ldc16,
                    int64_t req_stride, int64_t row0, void* stream);
int ot_attn_fwd_cached_kv16(const float* qkv, int64_t ld, const uint16_t* kv16, int64_t ldc16, int64_t req_stride,
                            const int32_t* req, int C, int H, int Ic, int n, int Kq, int head_dim,
                            const uint8_t* cache_valid, int64_t ldcv, float* out, float* lse_or_null, void* stream);

/* ---- pyramid query selection (pyramid.hip) -----------------------------------------------
 * Replaces PyramidScheduler.get_layer_config + tf.gather (model.py:287-302, 356, 371): per sample,
 * keep the K of I tokens with the largest key (score[b*I+p] * score_sign, ties to the later
 * position), the last `nforce` (<= K) positions always kept, positions emitted ascending.  score NULL =
 * every score equal = the reference's tail slice (range(I-K, I), D2-fixed).  One wavefront per
 * sample: bitwise radix select of the K-th key by ballot/popcount, ordered compaction by mbcnt.
 * pos [B*K]: kept positions; inv [B*I] (optional): compact row b*K+j of token row b*I+p, or -1;
 * map_rows (optional): map_rows[b*map_per_sample + j] = b*I + pos[b*K+j] for j < map_per_sample
 * (rewrites the shared-group part of a tail row map, layout.layer_maps).  I <= 4096. */
int ot_pyramid_select(const float* score, float score_sign, int B, int I, int K, int nforce,
                      int32_t* pos, int32_t* inv, int32_t* map_rows, int map_per_sample, void* stream);

/* ---- row-wise kernels (rowwise.hip) -------------------------------------------------------
 * RMSNorm model.py:19-23 (forward writes rstd, and y only when asked: the output norm
 * model.py:384); dropout model.py:184/193/198. */
int ot_rmsnorm_fwd(const float* x, int64_t ldx, const float* gamma, float* y, int64_t ldy, float* rstd,
                   int64_t rows, int d, float eps, void* stream);
size_t ot_rmsnorm_bwd_workspace_size(int64_t rows, int d);
/* dres (residual-branch gradient added to dx): when dres_tail_K > 0 it holds only the compact tail
 * rows (last dres_tail_K of every dres_tail_I rows of x); the other rows get no residual term. */
int ot_rmsnorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                   const float* rstd, const float* dres, int64_t lddres, int dres_tail_K, int dres_tail_I,
                   const int32_t* dres_tail_inv, float* dx, int64_t lddx,
                   float* dx_masked, int64_t lddxm, uint32_t seed, uint32_t site, float drop_rate,
                   int tail_K, int tail_I, const int32_t* tail_pos, float* dgamma, int accumulate_dgamma, int64_t rows, int d,
                   void* workspace, size_t ws_bytes, void* stream);
int ot_dropout_apply(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int d,
                     uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                     const int32_t* tail_pos, void* stream);
/* ot_dropout_apply that also reports the output's magnitude for fp16-pair consumers: amax (optional, one float the
 * caller zeroes) = max(*amax, max |out|) (atomic, order-independent); rowmax (optional, [rows][rowmax_n], rowmax_n =
 * ceil(d / 256)) = max |out| of each row's 256-column parts, only where ot_dropout_rowmax_supported(d) is 1 (d / 4 a
 * power of two or a multiple of 64; elsewhere a rowmax is refused and ot_rows_absmax stands in) */
int ot_dropout_rowmax_supported(int d);
int ot_dropout_apply_ex(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int d,
                        uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                        const int32_t* tail_pos, float* amax, float* rowmax, int rowmax_n, void* stream);
/* out[r][j] = max |x[r][c]| over c in [256 j, 256 j + 256) (parts = ceil(d / 256)): the row bounds (a_rowmax) of an
 * fp16-pair GEMM whose A has no producer that reports them */
int ot_rows_absmax(const float* x, int64_t ldx, int64_t rows, int d, float* out, int parts, void* stream);
/* ot_dropout_apply with the masked rows stored rounded to bf16 (uint16 bits, ldd in elements): the bf16
 * mode's dY of the FFN2 GEMM, whose consumers (the FFN2 dgrad's A operand, the W2 weight gradient's D)
 * round it to bf16 anyway */
int ot_dropout_apply_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t rows, int d,
                          uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                          const int32_t* tail_pos, void* stream);
size_t ot_rows_colsum_workspace_size(int64_t nrows, int ncols);
int ot_rows_colsum(const float* src, int64_t ld, const int32_t* rows, int64_t nrows, int ncols,
                   float* out, int accumulate, void* workspace, size_t ws_bytes, void* stream);

/* ---- tokenizer + heads + loss (model_io.hip) ---------------------------------------------- */
typedef struct {
  const float* dense;   /* [B] float feature (stride dense_stride) or NULL */
  const int64_t* ids;   /* [B] ids (stride ids_stride) for an embedding feature, or NULL */
  int64_t row_offset;   /* row of id 0 in the (concatenated) table */
  int64_t stride;       /* element stride between samples of `dense` / `ids` */
  int col;              /* first destination column */
  int width;            /* 1 for dense, embedding width for ids */
} ot_ns_field;
/* NS feature concat model.py:243-253 (+ embedding gather for id features):
 * out[b][col .. col+width) = table[row_offset + ids[b]] or dense[b]; columns >= F are untouched. */
int ot_ns_assemble(const ot_ns_field* fields_dev, int nfields, const float* table, int B, float* out,
                   int64_t ld_out, void* stream);
/* Pack the NS embedding-feature gradients of ot_ns_assemble: keys[f*B + b] = row_offset+ids[b],
 * grads[f*B + b][:] = dmat[b][col .. col+width) for the nsparse id fields (equal width). */
int ot_ns_grad_pack(const ot_ns_field* fields_dev, int nsparse, int width, const float* dmat, int64_t ld,
                    int B, int64_t* keys, float* grads, void* stream);
/* [SEP] placement model.py:270-272: dst[rows[i]][:] = vec[:] */
int ot_fill_rows(float* dst, int64_t ld, const int32_t* rows, int64_t nrows, const float* vec, int d,
                 void* stream);
/* Row maps of the per-sequence projection GEMM model.py:262-265: in_rows[m] = ids (item id) of
 * sequence element m; sequences concatenated, tiles padded to ot_gemm_tile_rows(). */
int ot_seq_rows(const int64_t* ids, int64_t ids_stride_b, int B, int L, int64_t vocab, int32_t* in_rows,
                void* stream);
/* Task heads model.py:388-391: logits[t][b] = gelu(pre1[t*B+b]) . w2[t] + b2[t], probs = sigmoid */
int ot_head_fwd(const float* pre1, const float* w2, const float* b2, int T, int B, int dh,
                float* logits, float* probs, void* stream);
size_t ot_head_bwd_workspace_size(int T, int B, int dh);
int ot_head_bwd(const float* pre1, const float* w2, const float* probs, const float* dprobs, int T, int B,
                int dh, float* dpre1, float* dw2, float* db2, int64_t task_stride_w2, int64_t task_stride_b2,
                int accumulate, void* workspace, size_t ws_bytes, void* stream);
/* ot_head_bwd with the loss gradient given w.r.t. the logits and / or the probabilities (either may be null):
 * dz = dlogits + dprobs * p (1 - p).  The model's training path passes dlogits (ot_task_loss_logits_bwd). */
int ot_head_bwd_ex(const float* pre1, const float* w2, const float* probs, const float* dprobs, const float* dlogits,
                   int T, int B, int dh, float* dpre1, float* dw2, float* db2, int64_t task_stride_w2,
                   int64_t task_stride_b2, int accumulate, void* workspace, size_t ws_bytes, void* stream);
/* The task loss of train.py:78-93 as the reference's Keras 2.12 evaluates it on its sigmoid heads (model.py:327-329,
 * train.py:84-87, 124-128): keras.activations.sigmoid caches its input as the output's _keras_logits and
 * keras.backend.binary_crossentropy(from_logits=False) then computes tf.nn.sigmoid_cross_entropy_with_logits:
 *   BCE task t:  mean_b  max(z, 0) - z y + log(1 + exp(-|z|))      (z = logits[t][b]; no clipping)
 *   MSE task t (bit t of mse_mask, tasks other than 'ctr' / 'cvr'):  mean_b (y - p)^2
 * loss = sum over the T <= 32 tasks.  Workspace: ot_bce_workspace_size.
 * bwd: dlogits = gscale[0] * d loss / d z = gscale (p - y) / B (BCE), gscale 2 (p - y) p (1 - p) / B (MSE). */
int ot_task_loss_logits_fwd(const float* logits, const float* probs, const float* labels, int T, int B,
                            unsigned mse_mask, float* loss, void* workspace, size_t ws_bytes, void* stream);
int ot_task_loss_logits_bwd(const float* probs, const float* labels, const float* gscale, int T, int B,
                            unsigned mse_mask, float* dlogits, void* stream);
/* The probability form (a caller holding only probabilities: Keras without a cached logit):
 * tf.keras.losses.BinaryCrossentropy(from_logits=False) summed over tasks,
 * loss = sum_t mean_b -(y log(clip(p)+eps) + (1-y) log(1-clip(p)+eps)). */
size_t ot_bce_workspace_size(int T, int B);
int ot_bce_fwd(const float* probs, const float* labels, int T, int B, float* loss, void* workspace,
               size_t ws_bytes, void* stream);
/* dprobs = gscale[0] * d loss / d probs (zero where p was clipped) */
int ot_bce_bwd(const float* probs, const float* labels, const float* gscale, int T, int B, float* dprobs,
               void* stream);
/* Per-task loss of train.py:78-93: task t is tf.keras.losses.MeanSquaredError (SUM_OVER_BATCH_SIZE:
 * mean_b (y - p)^2) when bit t of mse_mask is set (tasks other than 'ctr'/'cvr'), the BCE above
 * otherwise; loss = sum over the T <= 32 tasks.  ot_bce_* == mse_mask 0.  Workspace: ot_bce_workspace_size. */
int ot_task_loss_fwd(const float* probs, const float* labels, int T, int B, unsigned mse_mask, float* loss,
                     void* workspace, size_t ws_bytes, void* stream);
int ot_task_loss_bwd(const float* probs, const float* labels, const float* gscale, int T, int B,
                     unsigned mse_mask, float* dprobs, void* stream);
/* ---- weighted task loss (model_io.hip) ------------------------------------------------------
 * Build extension (Keras's sample_weight / loss_weights; no reference site).  l[t][b] is the per-element term of
 * the calls above: the logits-form BCE (logits given), the clipped probability-form BCE (logits NULL), or
 * (y - p)^2 for a task whose bit is set in mse_mask.
 *   weights      task t's B weights at + t * weight_stride; weight_stride 0 = one [B] row shared by all tasks,
 *                otherwise >= B.  A weight is clamped to [0, OT_LOSS_WEIGHT_MAX]; a NaN or a negative value is 0.
 *                A zero weight removes the entry by selection: its label and prediction do not enter the loss,
 *                whatever they hold (NaN, +-inf), and its gradient is exactly 0.
 *   task_scale   T coefficients a_t (device memory), or NULL for ones
 *   reduction    OT_LOSS_REDUCE_BATCH:   loss = sum_t a_t (sum_b w l) / B     (Keras SUM_OVER_BATCH_SIZE)
 *                OT_LOSS_REDUCE_WEIGHTS: loss = sum_t a_t (sum_b w l) / sum_b w; a task whose weights sum to 0
 *                contributes loss 0 and gradient 0
 *   denom        [T] floats, written by fwd (B or sum_b w) and read by bwd: no host sync in between
 * fwd: grid (workgroups, T), per-task partials {sum w l, sum w} in the workspace
 * (ot_task_loss_weighted_workspace_size), folded in index order in double: run-to-run bit-identical.
 * bwd: dout[t][b] = gscale[0] a_t w dl/dz / denom_t (prob_form 0: to the logits) or ... dl/dp ... (prob_form 1: to
 * the probabilities, 0 where p was clipped).  T <= 32, B >= 1. */
#define OT_LOSS_REDUCE_BATCH 0
#define OT_LOSS_REDUCE_WEIGHTS 1
#define OT_LOSS_WEIGHT_MAX 65536
size_t ot_task_loss_weighted_workspace_size(int T, int B);
int ot_task_loss_weighted_fwd(const float* logits, const float* probs, const float* labels, const float* weights,
                              int64_t weight_stride, const float* task_scale, int T, int B, unsigned mse_mask,
                              int reduction, float* loss, float* denom, void* workspace, size_t ws_bytes,
                              void* stream);
int ot_task_loss_weighted_bwd(const float* probs, const float* labels, const float* weights, int64_t weight_stride,
                              const float* task_scale, const float* denom, const float* gscale, int T, int B,
                              unsigned mse_mask, int prob_form, float* dout, void* stream);

/* ---- sparse embedding update (embedding.hip) ----------------------------------------------
 * Build extension (no reference site; paper: sparse Adagrad, clip 120, complete_translation.md:190).
 * Keras-2.12 Adagrad on a de-duplicated gradient: rows sorted (rocPRIM radix sort, stable) and
 * summed per unique key in a fixed order (deterministic), clip_by_norm(clip) over the unique-row
 * gradient, then acc[r] += g^2; w[r] -= lr g / sqrt(acc[r] + eps). */
size_t ot_sparse_adagrad_workspace_size(int64_t n, int E);
int ot_sparse_adagrad(float* table, float* accum, int E, int64_t num_rows, const int64_t* keys,
                      const float* grads, int64_t n, float lr, float eps, float clip,
                      void* workspace, size_t ws_bytes, void* stream);
/* Data-parallel form for replicated tables small enough to exchange densely (all-reduce instead of
 * an all-gather of every rank's rows): dense[key] = sum of the rows of key (dense zeroed by the
 * caller; same de-duplication as ot_sparse_adagrad, workspace ot_sparse_adagrad_workspace_size),
 * then clip_by_norm + Keras Adagrad over all rows (zero-gradient rows stay bitwise unchanged, i.e.
 * the same update as the sparse path). */
int ot_sparse_grad_dense(int E, int64_t num_rows, const int64_t* keys, const float* grads, int64_t n,
                         float* dense, void* workspace, size_t ws_bytes, void* stream);
size_t ot_dense_adagrad_workspace_size(void);
int ot_dense_adagrad(float* table, float* accum, const float* grad, int64_t num_rows, int E, float lr,
                     float eps, float clip, void* workspace, size_t ws_bytes, void* stream);
/* Two-phase sparse update for row-sharded tables (the clip norm spans all owners): prepare
 * de-duplicates and writes this rank's squared norm to sumsq_out (device float); the caller
 * all-reduces it; finish applies clip_by_norm(clip) with the global norm + Keras Adagrad.  Same
 * workspace (ot_sparse_adagrad_workspace_size) for both calls. */
int ot_sparse_prepare(int E, int64_t num_rows, const int64_t* keys, const float* grads, int64_t n, float* sumsq_out,
                      void* workspace, size_t ws_bytes, void* stream);
int ot_sparse_finish(float* table, float* accum, int E, int64_t n, float lr, float eps, float clip,
                     const float* sumsq_total, void* workspace, size_t ws_bytes, void* stream);
/* Row-wise Adagrad (optimizer_config['sparse_optimizer'] = 'rowwise_adagrad'): one accumulator per table row,
 * accum_rows [num_rows] f32, instead of one per element.  The same de-duplication, fixed summation order and
 * clip_by_norm as the three forms above, then for every unique valid key r with clipped row g
 *   accum_rows[r] += (sum_c g[c]^2) / E ;  w[r, c] -= lr g[c] / sqrt(accum_rows[r] + eps).
 * The row's sum of squares is added in an order fixed by E alone (no atomics), the same in the three forms: with
 * the clip off they give the same bits, run to run and form to form.  A row no valid key names (dense form: a row
 * whose clipped gradient is all zeros) keeps its weight and accumulator bits.  E: a multiple of 4, <= 1024, in all
 * three.  Workspaces as for the element-wise forms (ot_sparse_adagrad_workspace_size: one call and finish, after
 * the unchanged ot_sparse_prepare; ot_dense_adagrad_workspace_size: dense). */
int ot_sparse_adagrad_rowwise(float* table, float* accum_rows, int E, int64_t num_rows, const int64_t* keys,
                              const float* grads, int64_t n, float lr, float eps, float clip, void* workspace,
                              size_t ws_bytes, void* stream);
int ot_dense_adagrad_rowwise(float* table, float* accum_rows, const float* grad, int64_t num_rows, int E, float lr,
                             float eps, float clip, void* workspace, size_t ws_bytes, void* stream);
int ot_sparse_finish_rowwise(float* table, float* accum_rows, int E, int64_t n, float lr, float eps, float clip,
                             const float* sumsq_total, void* workspace, size_t ws_bytes, void* stream);

/* ---- row-sharded embedding tables (shard.hip) ------------------------------
 * Row id lives on rank id % world at local row id / world.  ot_shard_route buckets n ids by owner
 * (stable): perm[j] = position of the j-th routed id, send_local[j] = its local row at the owner
 * (-1 for ids outside [0, num_rows)), counts[r] = ids routed to rank r.  The all-to-all exchanges
 * are the caller's (RCCL); ot_gather_rows / ot_permute_rows move the rows on each side. */
size_t ot_shard_route_workspace_size(int64_t n);
int ot_shard_route(const int64_t* ids, int64_t n, int64_t num_rows, int world, int32_t* perm, int64_t* send_local,
                   int32_t* counts, void* workspace, size_t ws_bytes, void* stream);
/* De-duplicating route (replaces ot_shard_route in ShardedTable.lookup; same owner rule): the n ids
 * sorted by (owner, local row), stable, with equal ids merged into U unique entries in owner order.
 * uniq_local[u] = local row of unique u at its owner (-1: every id outside [0, num_rows) merges into
 * one entry routed to rank 0); counts[r] = unique ids owned by rank r (U = their sum); inv[i] = the
 * unique entry of id i (int64: the idx of ot_gather_rows that expands the U fetched rows to the n
 * tokens); order[j] = position of the j-th id in sorted order and run_start[u] = first j of unique
 * u (run_start[U] = n), the runs of ot_segment_rows_sum.  Arrays sized n (run_start n + 1). */
size_t ot_shard_route_unique_workspace_size(int64_t n);
int ot_shard_route_unique(const int64_t* ids, int64_t n, int64_t num_rows, int world, int64_t* uniq_local,
                          int64_t* inv, int32_t* order, int32_t* run_start, int32_t* counts, void* workspace,
                          size_t ws_bytes, void* stream);
/* out[u] = sum of src[order[j]] for j in [run_start[u], run_start[u+1]), ascending j (deterministic):
 * the per-token gradient rows of a de-duplicated route summed per unique id before they travel */
int ot_segment_rows_sum(const float* src, const int32_t* order, const int32_t* run_start, int64_t U, int E,
                        float* out, void* stream);
/* The same sums, balanced for Zipf-hot ids (runs cut into pieces of <= 64 positions, piece partials added
 * in piece order: deterministic); n = the routed id count (run_start[U]).  ws:
 * ot_segment_rows_sum_workspace_size(U, n, E) bytes. */
size_t ot_segment_rows_sum_workspace_size(int64_t U, int64_t n, int E);
int ot_segment_rows_sum_ex(const float* src, const int32_t* order, const int32_t* run_start, int64_t U, int64_t n,
                           int E, float* out, void* workspace, size_t ws_bytes, void* stream);
/* out[i] = table[idx[i]] (zeros for idx < 0) */
int ot_gather_rows(const float* table, int E, const int64_t* idx, int64_t n, float* out, void* stream);
/* inverse = 0: dst[j] = src[perm[j]]; inverse = 1: dst[perm[j]] = src[j] */
int ot_permute_rows(const float* src, const int32_t* perm, int64_t n, int E, int inverse, float* dst, void* stream);
/* shard init U(lo, hi) from a counter-based hash of (global row, column): the same logical table
 * for every world size */
int ot_hash_uniform_rows(float* out, int64_t local_rows, int E, int rank, int world, uint32_t seed, float lo,
                         float hi, void* stream);

/* ---- dense optimizer (optim.hip) ----------------------------------------------------------
 * Per-variable tf.clip_by_norm (train.py:134-135) over 2-D strided segments of one flat
 * gradient buffer, then Keras-2.12 RMSprop(momentum) (train.py:64-70, 138):
 *   v = rho v + (1-rho) g^2; inc = lr g rsqrt(v + eps); m = mom m + inc; w -= m.
 * segs: [nseg][4] int64 {offset, rows, cols, row_stride}. */
size_t ot_clip_rmsprop_workspace_size(int nseg, int64_t max_seg_elems);
int ot_clip_rmsprop(float* w, float* g, float* v, float* m, const int64_t* segs_dev, int nseg,
                    int64_t max_seg_elems, float lr, float rho, float eps, float momentum, float clip,
                    void* workspace, size_t ws_bytes, void* stream);
/* The same clip over the same segments, then Keras-2.12 Adam (train.py:57-63; 71-74 with the Keras defaults):
 *   alpha = lr sqrt(1 - beta2^step) / (1 - beta1^step)      (host, double)
 *   m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); w -= (m alpha) / (sqrt(v) + eps)
 * eps is outside the square root (RMSprop above: inside).  step >= 1 is the index of the step being applied
 * (Keras' iterations + 1); 0 <= beta1 < 1; 0 <= beta2 <= 1 (beta2 == 1: alpha = 0, w and v keep their bits, m
 * moves).  Elements outside every segment are not touched.  No host sync; deterministic. */
size_t ot_clip_adam_workspace_size(int nseg, int64_t max_seg_elems);
int ot_clip_adam(float* w, float* g, float* m, float* v, const int64_t* segs_dev, int nseg,
                 int64_t max_seg_elems, float lr, float beta1, float beta2, float eps, int64_t step, float clip,
                 void* workspace, size_t ws_bytes, void* stream);

/* ---- streaming metrics (metrics.hip) -------------------------------------------------------
 * The running Keras metrics the reference updates in every train / validation step (train.py:95-109,
 * 140-150, 176-185; evaluate.py:39-56) as additive device state, updated by one stream-ordered call:
 * no sync, no allocation, graph-capturable.  The caller zeroes the state to reset it and finalises
 * the metrics on the host (recommend_amd/metrics.py).
 *   probs, labels  task t's B values at + t * task_stride (the [T, B] layout of the model's
 *                  probabilities and of the stacked labels); task_stride >= B; any float alignment
 *                  (16-byte vector loads when both rows allow them, scalar loads otherwise: the
 *                  result does not depend on which)
 *   bounds         nb thresholds, ascending, doubles, device memory; 1 <= nb <= 1024
 *   counts         [T][2][nb+1] int64, += : class = (label > 0.5); bin = the number of j with
 *                  (double)p > bounds[j] (strict, as Keras's pred > threshold; a NaN is greater
 *                  than nothing: bin 0).  Exact: a per-workgroup LDS histogram, its non-zero
 *                  bins flushed with 64-bit integer atomics.
 *   sums           [T][4] double, += : {n, sum (p-y)^2, sum |p-y|, sum bce}, each term in double
 *                  from the f32 inputs; bce = -(y log(c+1e-7) + (1-y) log(1-c+1e-7)),
 *                  c = p clipped to [1e-7, 1-1e-7] (tf.keras.losses.BinaryCrossentropy on
 *                  probabilities).  Bit-reproducible: fixed-order reduction inside a workgroup,
 *                  workgroup partials folded in index order through the workspace; no float
 *                  atomics.
 * Every task gets every statistic (the host picks what it reports).  T <= 32, B >= 1. */
size_t ot_metrics_workspace_size(int T, int B);
int ot_metrics_update(const float* probs, const float* labels, int T, int B, int64_t task_stride,
                      const double* bounds, int nb, int64_t* counts, double* sums, void* workspace,
                      size_t ws_bytes, void* stream);
/* The weighted sibling (Keras metrics under sample_weight): the same walk with a third operand.
 *   weights        task t's B weights at + t * weight_stride (0 = one [B] row for every task, otherwise >= B),
 *                  clamped to [0, 2^16] (NaN, negatives: 0) and rounded to the nearest multiple of 2^-24: u units,
 *                  OT_METRICS_WEIGHT_ONE units = weight 1.  A sample of 0 units is skipped whatever it holds.
 *   counts         += u per sample instead of 1 (a per-workgroup 64-bit LDS histogram, touched bins flushed with
 *                  64-bit integer atomics): exact and commutative like the un-weighted state
 *   sums           += {sum u (added as integers per call), sum u (p-y)^2, sum u |p-y|, sum u bce}; the last three in
 *                  double in the fixed order above; no float atomics
 * A state updated this way is in units throughout: every reported ratio is the un-weighted formula on it.  Exact
 * while a window's sum of weights stays under 2^29 (sum u < 2^53).  Workspace: ot_metrics_weighted_workspace_size. */
#define OT_METRICS_WEIGHT_ONE (1 << 24)
size_t ot_metrics_weighted_workspace_size(int T, int B);
int ot_metrics_update_weighted(const float* probs, const float* labels, const float* weights, int T, int B,
                               int64_t task_stride, int64_t weight_stride, const double* bounds, int nb,
                               int64_t* counts, double* sums, void* workspace, size_t ws_bytes, void* stream);

/* ---- grouped AUC (metrics_grouped.hip) -----------------------------------------------------
 * The impression-weighted user-level AUC (UAUC) of the paper (complete_translation.md:178-180) over
 * a window of n records (group id, label, score), per binary task; stream-ordered, no allocation,
 * no host sync.  For one task, over records (g_i, y_i, s_i):
 *   class        y_i > 0.5, as in the streaming metrics above
 *   score order  the order of the f32 values; -0.0 ties with +0.0; every NaN ties with every other
 *                NaN and ranks above +inf
 *   per group u  n_pos, n_neg, and 2U = sum over (pos p, neg q) in u of (2 [s_p > s_q] + [s_p == s_q]),
 *                an exact integer (= sum over pos of (a + b + 1 - 2 start_u) - n_pos (n_pos + 1), [a, b)
 *                the element's tie run in the (group, score)-sorted order)
 *   valid        n_pos > 0 and n_neg > 0; then AUC_u = (double)2U / (2.0 n_pos n_neg)
 *   UAUC         sum_valid n_u AUC_u / sum_valid n_u, n_u = n_pos + n_neg (the caller divides: agg[0] /
 *                agg[2], 0 with no valid group)
 * Operands:
 *   groups       [n] int64 ids (compared as unsigned 64-bit); group_bits (1..64) is the caller's promise
 *                that every id is below 2^group_bits: it only shortens the sort
 *   scores, labels  task t's n values at + t * task_stride (task_stride >= n), any float alignment
 *   task_mask    bit t set: task t is binary and is computed; a clear bit leaves its agg row and its
 *                group_stats zero
 *   agg          [T][4] double, overwritten: {sum n_u AUC_u, sum AUC_u, sum n_u, number of valid groups}
 *   num_groups   [1]: the number G of distinct ids
 *   group_ids    [n] or NULL: the G distinct ids, ascending as unsigned 64-bit (the rest is not written)
 *   group_stats  [T][n][3] or NULL: {n_pos, n_neg, 2U} of each distinct group in the same order, the
 *                rows from G on zero
 * The per-group integers are exact (64-bit integer accumulation, which commutes).  agg is reduced in a
 * fixed order over the groups in ascending id order (thread -> wave -> workgroup -> workgroups in
 * index order, no float atomics): bit-identical from run to run and under any permutation of the
 * records.  1 <= T <= 32, 1 <= n < 2^31.  The workspace takes about 40 bytes per record plus the
 * sort's scratch. */
size_t ot_grouped_auc_workspace_size(int T, int64_t n, int group_bits);
int ot_grouped_auc(const int64_t* groups, const float* scores, const float* labels, int T, int64_t n,
                   int64_t task_stride, int group_bits, uint32_t task_mask, double* agg,
                   int64_t* num_groups, int64_t* group_ids, int64_t* group_stats, void* workspace,
                   size_t ws_bytes, void* stream);

/* ---- ranking (rank.hip) --------------------------------------------------------------------
 * Per-request top-K of scored candidates, the serving step after stage II: C candidates with T task
 * probabilities each and a request index, R requests, K slots per request; stream-ordered, no
 * allocation, no host sync, no device-to-host copy.
 *   probs        f32, task t's C values at + t * task_stride (task_stride >= C): the head's [T, C]
 *   weights_host T host floats, read at call time and passed to the kernel by value
 *   fused score  f[c], f32, in task order t = 0..T-1 with one rounding per step:
 *                  OT_RANK_SUM      f = fmaf(w_t, p_t, f) from 0.0f (T = 1, w = 1: the bits of p)
 *                  OT_RANK_PRODUCT  f = f * p_t over the tasks with w_t != 0, from 1.0f
 *   order        orderable(f) = 0 for a NaN; else with u = bits(f + 0.0f) (-0 ties with +0),
 *                (u & 0x80000000) ? ~u : (u | 0x80000000).  A NaN ranks below -inf.  The 64-bit key is
 *                orderable(f) << 32 | (0xFFFFFFFF - c): keys are distinct, a higher score wins and equal
 *                scores go to the lower candidate index.
 *   membership   candidate c belongs to request req[c] when 0 <= req[c] < R.  Any other value excludes
 *                it (the way to mask filtered candidates): it is never used as an index and appears in
 *                no row.
 *   outputs      for request r with n_r members and k_r = min(K, n_r):
 *                  top_idx   [R][K] int32: [r][0..k_r) the candidates of the k_r largest keys, in
 *                            descending key order; the slots from k_r on are -1
 *                  top_score [R][K] f32: f[top_idx], bit for bit (a NaN included); the slots from k_r on
 *                            are -inf
 *                  count     [R] int32: k_r
 *                  fused_out [C] f32 or NULL: f of every candidate, excluded ones included
 * The answer is unique, so the outputs are bit-identical from run to run and under any arrival order
 * of the integer atomics inside.  1 <= K <= 1024, 1 <= T <= 32, 0 <= C <= INT32_MAX, R >= 0; R = 0 or
 * C = 0 writes the empty answer (every slot padding, every count 0).  The workspace takes 16 bytes per
 * candidate and 8 per request. */
#define OT_RANK_SUM 0
#define OT_RANK_PRODUCT 1
size_t ot_rank_topk_workspace_size(int R, int64_t C, int K);
int ot_rank_topk(const float* probs, int64_t task_stride, int T, const float* weights_host, int mode,
                 const int32_t* req, int64_t C, int R, int K, int32_t* top_idx, float* top_score,
                 int32_t* count, float* fused_out, void* workspace, size_t ws_bytes, void* stream);

/* ---- sequence fusion (seqfuse.hip) ------------------------------------------------------------
 * Timestamp-aware fusion of a sample's behaviour sequences into one token stream: the output-row
 * entries of the per-sequence projection GEMM's row map, computed per call from the events' times.
 * Stream-ordered, no allocation, no host sync.
 *   seqs      nseq HOST descriptors, read at call time and passed to the kernel by value; their order
 *             is the order of the sequences in the key below.  times: device int64, sample b's L events
 *             at times + b * stride_b (stride_b >= L); map_off: first entry of the sequence's segment
 *             in out_rows (the segment offsets ot_seq_rows is given); L may be 0.  sum of L = L_S.
 *   order     per sample, the stable sort of its L_S events by the key (time, index of the sequence
 *             in seqs, position in the sequence): a total order, so the ranks are a permutation of
 *             0 .. L_S-1 for any times (unsorted sequences, ties, all equal).  Times compare as signed
 *             64-bit integers: INT64_MIN, the value for padding events, sorts first.
 *   outputs   for event j of sequence i in sample b, with rank its place in that order:
 *               out_rows[map_off_i + b * L_i + j] = b * row_stride + rank   (row_stride >= L_S)
 *               rank_out[b * L_S + start_i + j]   = rank   (start_i = L_0 + .. + L_{i-1}; or NULL)
 *               last_time[b]                      = the sample's largest time           (or NULL)
 *             No other entry of out_rows is written: the map's -1 padding stays.
 * 1 <= nseq <= 32, B >= 0, 1 <= L_S <= 4096 (the keys are sorted in LDS, 12 bytes per event),
 * B * row_stride <= INT32_MAX; anything else, inconsistent descriptors or a workspace below
 * ot_seq_time_rows_workspace_size return OT_ERR_INVALID_ARG without launching.  B = 0 is a no-op.
 * The sort needs no scratch memory today: the workspace size is one 256-byte unit for every valid
 * shape (0 for an invalid one). */
typedef struct {
  const int64_t* times; /* device, [B] rows of L times, row stride stride_b */
  int64_t stride_b;
  int32_t L;            /* events per sample */
  int32_t map_off;      /* the sequence's segment offset in out_rows */
} ot_seq_time;
size_t ot_seq_time_rows_workspace_size(int B, int nseq, int L_S);
int ot_seq_time_rows(const ot_seq_time* seqs, int nseq, int B, int L_S, int64_t row_stride, int32_t* out_rows,
                     int32_t* rank_out, int64_t* last_time, void* workspace, size_t ws_bytes, void* stream);

/* ---- embedding bags (bag.hip) -----------------------------------------------------------------
 * Multi-valued NS id features pooled into one column block of the NS concat matrix each, and the
 * (key, gradient row) pairs of their slots for ot_sparse_adagrad.  Stream-ordered, no allocation, no
 * host sync, no atomics: results are bitwise reproducible.
 *   bags      nbags HOST descriptors (1 .. OT_NS_BAG_MAX), read at call time and passed to the kernel by
 *             value.  ids: device int64, sample b's cap slots at ids + b * ids_stride; a slot whose id is
 *             outside [0, num_rows) is EMPTY: never read, coefficient 0, key -1.  weights: NULL, or device
 *             f32 per slot at weights + b * weights_stride (pooling OT_BAG_SUM only).  table: device f32
 *             rows of `width` floats, 16-byte aligned; the caller vouches that rows row_offset ..
 *             row_offset + num_rows - 1 exist.  Strides are in elements, >= cap.
 *   pool      out[b][col .. col + width) = sum over the valid slots of coef * table[row_offset + id],
 *             coef = w_j * s_b, w_j = 1 without weights, s_b = 1 (SUM) or 1.0f / (valid slots of the
 *             bag) (MEAN); an empty bag gives zeros.  Every other column of out is untouched.
 *             coef_out[base_f + b * cap_f + j] = that coefficient (0 for an empty slot), base_f = B * (cap_0
 *             + .. + cap_{f-1}) over the descriptors of THIS call: sum of B * cap floats.
 *   grad_pack the bags of one table (equal width E; `table` is not read): for slot position p = base_f +
 *             b * cap_f + j, keys[p] = row_offset + id or -1 (empty), grads[p][c] = coef[p] * dmat[b][col + c]
 *             (one f32 multiply; zeros for an empty slot).  coef: the pool's coef_out, at the first
 *             descriptor's base.  grads 16-byte aligned.
 * width % 4 == 0 and width <= OT_NS_BAG_MAX_WIDTH, cap >= 1, col + width <= ld, B * cap < 2^31 in total;
 * anything else, or a null operand, returns OT_ERR_INVALID_ARG without launching.  B = 0 is a no-op. */
#define OT_NS_BAG_MAX 32
#define OT_NS_BAG_MAX_WIDTH 256
#define OT_BAG_SUM 0
#define OT_BAG_MEAN 1
typedef struct {
  const float* table;     /* device, rows of `width` floats */
  const int64_t* ids;     /* device, [B] rows of cap ids, row stride ids_stride */
  const float* weights;   /* device, [B] rows of cap weights, row stride weights_stride, or NULL */
  int64_t row_offset;     /* row of id 0 in the table */
  int64_t num_rows;       /* ids outside [0, num_rows) are empty slots */
  int64_t ids_stride;
  int64_t weights_stride;
  int32_t width;          /* E */
  int32_t cap;            /* slots per sample */
  int32_t col;            /* first destination column */
  int32_t pooling;        /* OT_BAG_SUM | OT_BAG_MEAN */
} ot_ns_bag;
int ot_ns_bag_pool(const ot_ns_bag* bags, int nbags, int B, float* out, int64_t ld_out, float* coef_out,
                   void* stream);
int ot_ns_bag_grad_pack(const ot_ns_bag* bags, int nbags, int B, const float* dmat, int64_t ld, const float* coef,
                        int64_t* keys, float* grads, void* stream);

/* ---- group-wise NS tokenizer (ns_group.hip) ------------------------------------------------------
 * Paper eq. 6: the NS features are partitioned into G groups and group g goes through its own
 * Dense(K_g -> d) to become NS token g; a grouped GEMM whose groups differ in K.  Every row b of the NS
 * matrix A feeds all G groups, group g from the columns goff[g] .. goff[g+1]-1 and the rows of the same
 * numbers of the group-major weight bank W [goff[G]][d]; bias is [G][d].
 *   fwd         X[b*ldx + g*d + n]      = sum_k A[b*lda + goff[g]+k] * W[(goff[g]+k)*d + n] + bias[g*d + n]
 *   bwd_input   dA[b*lda + goff[g]+k]   = sum_n D[b*ldd + g*d + n] * W[(goff[g]+k)*d + n]   (every column of
 *               every group's range is written; columns of A outside the ranges are untouched)
 *   bwd_weight  dW[(goff[g]+k)*d + n] (+)= sum_b A[b*lda + goff[g]+k] * D[b*ldd + g*d + n],
 *               db[g*d + n] (+)= sum_b D[b*ldd + g*d + n]; row chunks write partial slabs into the workspace
 *               (ot_ns_group_wgrad_workspace_size) and the slabs are added in chunk order: bitwise
 *               reproducible, no float atomics.  accumulate != 0 adds onto dW / db.
 * goff: DEVICE int32 [G+1], goff[0] = 0, strictly increasing (no alignment is assumed); the host passes G,
 * ktot = goff[G] and kmax >= the largest K_g = goff[g+1] - goff[g].  goff is never read on the host: a range
 * that is empty or leaves [0, ktot] is skipped on the device, so no table can send an access out of bounds.
 * Arithmetic: exact f32, one fmaf per product in ascending order of the summed index, whatever the model's
 * matmul precision.  Stream-ordered, no allocation, no host sync.
 * B >= 1, G >= 1, d % 4 == 0 and 4 <= d <= 512, ktot <= 2^22, lda >= ktot, ldx / ldd >= G*d and a multiple
 * of 4, W / bias / X / D / dW / db / workspace 16-byte aligned; anything else, or a null operand, returns
 * OT_ERR_INVALID_ARG before any launch. */
int ot_ns_group_fwd(const float* A, int64_t lda, const int32_t* goff, int G, int ktot, int kmax, const float* W,
                    const float* bias, int B, int d, float* X, int64_t ldx, void* stream);
int ot_ns_group_bwd_input(const float* D, int64_t ldd, const int32_t* goff, int G, int ktot, int kmax,
                          const float* W, int B, int d, float* dA, int64_t lda, void* stream);
size_t ot_ns_group_wgrad_workspace_size(int B, int G, int ktot, int d);
int ot_ns_group_bwd_weight(const float* A, int64_t lda, const float* D, int64_t ldd, const int32_t* goff, int G,
                           int ktot, int kmax, int B, int d, float* dW, float* db, int accumulate, void* workspace,
                           size_t ws_bytes, void* stream);

/* ---- probe of the scaled fp16-pair split (pair_probe.hip; a test hook, on no hot path) -------------------
 * The two fp16 planes (bit patterns) the pair GEMMs form from an f32 operand: with t = f32(x[i] * scale),
 *   form 0 (the plane GEMMs' and the fused FFN's split): t saturated to [-65504, 65504] (a NaN stays a NaN),
 *   form 1 (the pair weight gradient's split) and form 2 (the slice attention's split): t as it is,
 * hi[i] = fp16(t), lo[i] = fp16(t - f32(hi[i])), both rounded to nearest even.  n is a multiple of 8 (form 0) or
 * 4 (forms 1, 2); x, hi, lo are 16-byte aligned device pointers.  Stream-ordered, no allocation. */
int ot_pair_split_probe(const float* x, int64_t n, float scale, int form, uint16_t* hi, uint16_t* lo,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONETRANS_HIP_H */
