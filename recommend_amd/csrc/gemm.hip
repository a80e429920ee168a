// Mixed-parameterisation grouped GEMM on gfx950 fp32 MFMA (v_mfma_f32_32x32x2_f32).
//
// Replaces the reference's per-token Dense loops (model.py:84-92 Q/K/V, model.py:154-161 FFN),
// the Wo Dense (model.py:117), the tokenizer Dense layers (model.py:211-219) and their
// gradients.  One launch covers every weight group: rows are listed per tile (row maps), every
// tile belongs to one group g and multiplies by W[g].
//
//   fwd  (NN): C[out_row] = epi( pro(A[in_row]) @ W[g] )          W[g] stored [K][N] (Keras)
//   dgrad(NT): C[out_row] = epi( A[in_row] @ W[g]^T )             W[g] stored [N][K]
//   wgrad    : dW[g] (+)= sum_rows pro(A[a_row])^T D[d_row], db[g] (+)= sum_rows D[d_row]
//
// Tile 128x128, BK 32, 256 threads = 4 waves (2x2), each wave 64x64 = 2x2 MFMA 32x32 blocks.
// LDS images are [row][BK+4] (k contiguous, 144-B row stride => conflict-free ds_read_b128 for
// 16 consecutive rows).  The k index inside an MFMA step is permuted (lane half h supplies
// k = 16h + s at step s) so each lane reads 4 consecutive k with one ds_read_b128.
//
// (the register-staged mixed_gemm_kernel, gemm_mixed.h)
//
// This file: the host dispatch (mixed_gemm_impl) of the forward and input-gradient GEMMs and the edge-tile forms of
// mixed_gemm_kernel.  Its whole-tile forms are in gemm_mixed.hip, the plane GEMMs in gemm_plane.hip and
// gemm_plane_wide.hip, their weight images in gemm_images.hip, the weight gradients in gemm_wgrad.hip; gemm.h
// holds what they share.
#include <algorithm>

#include "gemm_mixed.h"

namespace ot {

// OT_EPI_ROW_RSTD with N > GT (plane GEMM): rstd_out[out_row] = rsqrt(sum of the row's ntn tile sums
// of squares / N + eps), tile sums added in column order (deterministic); one thread per tile row.
__global__ __launch_bounds__(256) void row_rstd_finish_kernel(const float* __restrict__ part, int ntn,
                                                              const int32_t* __restrict__ out_rows, int64_t nrows,
                                                              int N, float eps, float* rstd_out) {
  const int64_t gr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gr >= nrows) return;
  const int orr = out_rows ? out_rows[gr] : (int)gr;
  if (orr < 0) return;
  float s = 0.f;
  for (int j = 0; j < ntn; ++j) s += part[gr * ntn + j];
  rstd_out[orr] = rsqrtf(s / (float)N + eps);
}


}  // namespace ot

using namespace ot;

static int mixed_gemm_impl(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                           int a_xform, const float* a_rstd, const float* a_gamma,
                           const float* W, int64_t w_gstride, int64_t ldw, int N,
                           const int32_t* tile_group, int ntiles,
                           const float* bias, int64_t bias_gstride,
                           float* C, int64_t ldc, const int32_t* out_rows, int epi,
                           const float* res, int64_t ldres, int res_tok,
                           const float* aux, int64_t ldaux,
                           uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                           const int32_t* tail_pos,
                           const ot_rms_epilogue* rms, const uint16_t* bimg, int bimg_ntn, int bimg_tn0,
                           int prec, void* stream) {
  OT_REQUIRE(prec == OT_MATMUL_F32 || prec == OT_MATMUL_SPLIT_BF16 || prec == OT_MATMUL_BF16,
             "ot_mixed_gemm: unknown precision %d", prec);
  OT_REQUIRE(A && W && C, "ot_mixed_gemm: null operand");
  const int rms_flags = epi & (OT_EPI_ROW_RSTD | OT_EPI_RMSNORM_BWD | OT_EPI_ROWDOT);
  OT_REQUIRE(!rms_flags || rms, "ot_mixed_gemm: row-norm epilogue flags need ot_mixed_gemm_rms");
  OT_REQUIRE(K > 0 && N > 0 && ntiles >= 0, "ot_mixed_gemm: bad sizes K=%d N=%d ntiles=%d", K, N, ntiles);
  OT_REQUIRE(K % 4 == 0 && lda % 4 == 0, "ot_mixed_gemm: K and lda must be multiples of 4");
  OT_REQUIRE(ldw % 4 == 0 && w_gstride % 4 == 0, "ot_mixed_gemm: ldw/w_gstride must be multiples of 4");
  OT_REQUIRE(mode == OT_GEMM_NN ? N % 4 == 0 : true, "ot_mixed_gemm: NN mode needs N %% 4 == 0");
  OT_REQUIRE(mode == OT_GEMM_NN || mode == OT_GEMM_NT, "ot_mixed_gemm: bad mode");
  OT_REQUIRE(!(epi & OT_EPI_BIAS) || bias, "ot_mixed_gemm: bias missing");
  OT_REQUIRE(!(epi & OT_EPI_RESIDUAL) || res, "ot_mixed_gemm: residual missing");
  OT_REQUIRE(!(epi & OT_EPI_GELU_BWD) || aux, "ot_mixed_gemm: aux missing");
  OT_REQUIRE(a_xform != OT_AX_RMSNORM || (a_rstd && a_gamma), "ot_mixed_gemm: rmsnorm prologue needs rstd/gamma");
  OT_REQUIRE(a_xform == OT_AX_NONE || a_xform == OT_AX_RMSNORM || a_xform == OT_AX_GELU || a_xform == OT_AX_BF16 ||
                 a_xform == OT_AX_BF16_RMSNORM,
             "ot_mixed_gemm: bad a_xform %d", a_xform);
  OT_REQUIRE(a_xform != OT_AX_BF16_RMSNORM || (a_rstd && a_gamma),
             "ot_mixed_gemm: OT_AX_BF16_RMSNORM needs rstd / gamma (gamma folded into the B image)");
  OT_REQUIRE((a_xform != OT_AX_BF16 && a_xform != OT_AX_BF16_RMSNORM) ||
                 (prec == OT_MATMUL_BF16 && bimg && mode == OT_GEMM_NT &&
                                       lda % 8 == 0 && ((uintptr_t)A % 16) == 0),
             "ot_mixed_gemm: OT_AX_BF16 (bf16 A) needs the bf16 mode, a B image (plane GEMM), NT mode and 16-B "
             "aligned rows");
  OT_REQUIRE(!rms || !rms->gelu_out || (((epi & OT_EPI_GELU_BWD) || (epi & ~OT_EPI_C_BF16) == OT_EPI_BIAS) &&
                                        rms->ldgelu % 4 == 0 &&
                                        ((uintptr_t)rms->gelu_out % 8) == 0),
             "ot_mixed_gemm_rms: gelu_out needs OT_EPI_GELU_BWD or epi == OT_EPI_BIAS, ldgelu %% 4 == 0 and 8-B "
             "alignment");
  OT_REQUIRE(!((epi & OT_EPI_DROPOUT) || res_tok) || (tail_K > 0 && tail_I >= tail_K), "ot_mixed_gemm: bad tail map");
  if (rms_flags) {
    OT_REQUIRE(mode == OT_GEMM_NT && N % GT == 0 &&
                   (N == GT || !(epi & OT_EPI_RMSNORM_BWD) || (rms->rowdot && rms->rowdot_n > 0)),
               "ot_mixed_gemm_rms: row-norm epilogues need NT mode and N %% %d == 0 (OT_EPI_RMSNORM_BWD with N > %d: "
               "the row-dot partials)", GT, GT);
    OT_REQUIRE(N == GT || !(epi & OT_EPI_ROW_RSTD) ||
                   (rms->workspace && rms->ws_bytes >= ot_mixed_gemm_rms_workspace_size(ntiles, N)),
               "ot_mixed_gemm_rms: OT_EPI_ROW_RSTD with N > %d needs the workspace", GT);
    OT_REQUIRE(!(epi & OT_EPI_ROWDOT) || ((epi & OT_EPI_GELU_BWD) &&
                                          !(epi & ~(OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16 | OT_EPI_AUX_BF16)) &&
                                          rms->rowdot && rms->rowdot_n == N / GT && bias),
               "ot_mixed_gemm_rms: OT_EPI_ROWDOT goes with OT_EPI_GELU_BWD only and needs rowdot[rows][N / %d] and "
               "the bias", GT);
    OT_REQUIRE(!(epi & OT_EPI_ROW_RSTD) || rms->rstd_out, "ot_mixed_gemm_rms: rstd_out missing");
    OT_REQUIRE(!(epi & OT_EPI_RMSNORM_BWD) || (rms->x && rms->gamma && rms->rstd && rms->ldx % 4 == 0),
               "ot_mixed_gemm_rms: RMSNorm backward needs x / gamma / rstd");
    OT_REQUIRE(!(epi & OT_EPI_RMSNORM_BWD) || !(epi & ~(OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT)),
               "ot_mixed_gemm_rms: RMSNorm backward combines with OT_EPI_DROPOUT only");
    OT_REQUIRE(!((epi & OT_EPI_RMSNORM_BWD) && (epi & OT_EPI_DROPOUT)) || rms->dx_masked,
               "ot_mixed_gemm_rms: dx_masked missing");
    OT_REQUIRE(!rms->dgamma || (rms->workspace && rms->ws_bytes >= ot_mixed_gemm_rms_workspace_size(ntiles, N)),
               "ot_mixed_gemm_rms: workspace too small");
    OT_REQUIRE(!rms->dres || rms->lddres % 4 == 0, "ot_mixed_gemm_rms: lddres must be a multiple of 4");
  }
  if (ntiles == 0) return OT_OK;
  GemmArgs p{A, lda, K, in_rows, a_xform, a_rstd, a_gamma, W, w_gstride, ldw, N, tile_group,
             bias, bias_gstride, C, ldc, out_rows, epi, res, ldres, res_tok, aux, ldaux,
             seed, site, 0u, 1.f, tail_K, tail_I, N, ntiles, (int)ceil_div(N, GT)};
  p.tail_pos = tail_pos;
  p.bimg = bimg; p.bimg_ntn = bimg_ntn; p.bimg_tn0 = bimg_tn0;
  float* dgpart = nullptr;
  if (rms && rms->xn_out) {
    p.xn_out = rms->xn_out;
    p.ldxn = rms->ldxn;
  }
  if (rms && rms->c16_out) {
    p.c16_out = rms->c16_out;
    p.ldc16 = rms->ldc16;
  }
  if (rms && rms->rowmax_out) {
    p.rowmax_out = rms->rowmax_out;
    p.rowmax_n = rms->rowmax_n;
  }
  if (rms) {
    p.amax_out = rms->amax_out;
    p.rowabs_out = rms->rowabs_out;
    p.rowabs_n = rms->rowabs_n;
  }
  if (rms && rms->a_rowmax && (a_xform == OT_AX_GELU || a_xform == OT_AX_NONE)) {
    p.a_rowmax = rms->a_rowmax;
    p.a_rowmax_n = rms->a_rowmax_n;
  }
  if (rms && ((epi & OT_EPI_GELU_BWD) || (epi & ~OT_EPI_C_BF16) == OT_EPI_BIAS)) {   // the stored GELU (optional)
    p.gelu_out = rms->gelu_out;
    p.ldgelu = rms->ldgelu;
  }
  if (rms_flags) {
    p.rstd_out = rms->rstd_out; p.eps = rms->eps;
    p.nx = rms->x; p.ldnx = rms->ldx; p.ngamma = rms->gamma; p.nrstd = rms->rstd;
    p.dres = rms->dres; p.lddres = rms->lddres; p.dres_K = rms->dres_tail_K; p.dres_I = rms->dres_tail_I;
    p.dres_inv = rms->dres_tail_inv;
    p.dxm = rms->dx_masked; p.lddxm = rms->lddxm;
    if ((epi & OT_EPI_ROW_RSTD) && N > GT) p.rowpart = (float*)rms->workspace;
    if ((epi & OT_EPI_ROWDOT) || ((epi & OT_EPI_RMSNORM_BWD) && N > GT)) {
      p.rowdot = rms->rowdot;
      p.rowdot_n = rms->rowdot_n;
    }
    if (epi & OT_EPI_RMSNORM_BWD) {
      // without dgamma the partials still need a home: the caller's workspace or nothing
      dgpart = rms->dgamma ? (float*)rms->workspace : nullptr;
      OT_REQUIRE(dgpart, "ot_mixed_gemm_rms: RMSNorm backward needs dgamma and its workspace");
      p.dgpart = dgpart;
    }
  }
  if (epi & OT_EPI_DROPOUT) {
    OT_REQUIRE(drop_rate >= 0.f && drop_rate < 1.f, "ot_mixed_gemm: drop_rate out of range");
    p.drop_thr = drop_threshold(drop_rate);
    p.drop_scale = 1.f / (1.f - drop_rate);
  }
  const bool split = prec != OT_MATMUL_F32 && mode == OT_GEMM_NT;
  const bool one = prec == OT_MATMUL_BF16;
  const size_t shmem = split ? 4 * GT * SRS * sizeof(uint16_t) : 4 * GT * GLD * sizeof(float);
  auto a16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  const bool vec_ok = ldc % 4 == 0 && a16(C) && (!(epi & OT_EPI_RESIDUAL) || (ldres % 4 == 0 && a16(res))) &&
                      (!(epi & OT_EPI_GELU_BWD) || (ldaux % 4 == 0 && a16(aux))) &&
                      (!(epi & (OT_EPI_BIAS | OT_EPI_ROWDOT)) || (bias_gstride % 4 == 0 && a16(bias)));
  const bool edge = (K % GBK) != 0 || (N % GT) != 0 || !vec_ok;
  OT_REQUIRE(!rms_flags || !edge, "ot_mixed_gemm_rms: needs K %% %d == 0 and 16-B aligned operands", GBK);
  const unsigned nwg = (unsigned)ntiles * p.ntn;
  hipStream_t s = (hipStream_t)stream;
  void (*kern)(GemmArgs) = nullptr;
  bool plane = false;
  int wide_lds = 0;                     // > 0: the wide / big / square plane GEMM (its stage LDS bytes, its kind)
  int wide_kind = 0;
  int panel_lds = 0;                    // > 0: the panel form of the pair plane GEMM (its LDS bytes)
  int plane_lds = 0;                    // plane_gemm_kernel's stage LDS bytes
  const int e = epi, x = a_xform;
  const int splt = split ? (one ? 1 : SPLIT_TERMS) : 0;
  const bool nt = mode == OT_GEMM_NT;
  kern = edge ? mixed_gemm_pick<true>(nt, x, e, splt) : mixed_gemm_whole_for(nt, x, e, splt);
  // plane GEMM: split mode, pre-split B image given, whole tiles, 16-B aligned A rows
  // (the plane GEMM's k-steps are 16 deep: K % 16 suffices, e.g. the NS tokenizer's K = 432)
  const bool plane_edge = (K % 16) != 0 || (N % GT) != 0 || !vec_ok;
  if (bimg && split && !plane_edge && mode == OT_GEMM_NT && lda % 4 == 0 && a16(A)) {
    OT_REQUIRE(bimg_ntn >= bimg_tn0 + (int)p.ntn && bimg_tn0 >= 0, "ot_mixed_gemm: B image has %d tiles per group, "
               "the GEMM needs %d from tile %d", bimg_ntn, (int)p.ntn, bimg_tn0);
    void (*pk)(GemmArgs) = plane_gemm_for(x, e, one, p.a_rowmax != nullptr, &plane_lds);
    if (pk) { kern = pk; plane = true; }
    p.rowmeta = pk && !one ? ot_plane_rowmeta(-1) : 0;   // (read by the TERMS-2 form)
    // pair (TERMS 2) launches with two or more column tiles: the panel form where it has the specialisation
    const bool pair = !one && (x == OT_AX_RMSNORM || (p.a_rowmax && x == OT_AX_NONE));
    const int pmode = ot_plane_panel(-1);
    if (pk && pair && p.ntn >= 2 && pmode) {
      const int pvar = pmode >= 200 ? (K == 128 ? 2 : 0) : pmode >= 100 ? 1 : 0;
      const int pwid = pmode == 1 ? plane_panel_width(ntiles, p.ntn) : std::min(std::max(pmode % 100, 2), (int)p.ntn);
      int lds = 0;
      void (*ppk)(GemmArgs) = pwid > 0 ? plane_panel_for(x, e, pvar, &lds) : nullptr;
      if (ppk) {
        kern = ppk;
        p.panel_w = pwid;
        panel_lds = lds;
      }
    }
    // bf16 mode, whole 256-column tiles and 32-k stages: the wide tile (same outputs)
    // tile: 1 auto, 2 / 3 / 4 force 128 x 256 / 128 x 512 / 256 x 256 (where the shape allows it)
    const int wmode = ot_plane_wide(-1);
    if (pk && one && wmode && N % PW_COLS == 0 && K % 32 == 0 && !(p.xn_out && K > 1024)) {
      int kind = wmode == 1 ? plane_tile_auto(K, N, ntiles) : wmode - 1;
      if (kind == 2 && N % PB_COLS != 0) kind = 1;
      if (kind == 3 && ntiles % 2 != 0) kind = 1;
      int stage_lds = 0;
      void (*wk)(GemmArgs) = kind ? plane_wide_for(x, e, kind, &stage_lds) : nullptr;
      if (wk) {
        kern = wk;
        wide_lds = stage_lds;
        wide_kind = kind;
      }
    }
  }
  OT_REQUIRE((x != OT_AX_BF16 && x != OT_AX_BF16_RMSNORM) || plane,
             "ot_mixed_gemm: no plane GEMM for a_xform %d with epilogue %d (or edge tiles)", x, epi);
  OT_REQUIRE(!p.c16_out || (plane && one && p.ldc16 % 4 == 0 && ((uintptr_t)p.c16_out % 8) == 0 &&
                            !(epi & (OT_EPI_RMSNORM_BWD | OT_EPI_C_BF16))),
             "ot_mixed_gemm_rms: c16_out needs the bf16-mode plane GEMM (not with OT_EPI_RMSNORM_BWD / C_BF16), "
             "ldc16 %% 4 == 0 and 8-B alignment");
  OT_REQUIRE(!(epi & (OT_EPI_C_BF16 | OT_EPI_AUX_BF16)) || plane,
             "ot_mixed_gemm: OT_EPI_C_BF16 / OT_EPI_AUX_BF16 need the bf16-mode plane GEMM with OT_EPI_GELU_BWD "
             "[| OT_EPI_ROWDOT] or OT_EPI_BIAS alone (epilogue %d)", epi);
  OT_REQUIRE(!p.gelu_out || (!edge && (kern != nullptr) && ((epi & OT_EPI_GELU_BWD) || (plane && one))),
             "ot_mixed_gemm_rms: gelu_out needs whole tiles (with epi OT_EPI_BIAS: the bf16-mode plane GEMM)");
  OT_REQUIRE(!p.xn_out || (plane && one && (x == OT_AX_RMSNORM || x == OT_AX_BF16_RMSNORM) && a_rstd && a_gamma &&
                           p.ldxn % 8 == 0 && K <= 1024 &&
                           ((uintptr_t)p.xn_out % 16) == 0),
             "ot_mixed_gemm_rms: xn_out needs the bf16-mode plane GEMM with the RMSNorm prologue, K <= 1024, ldxn %% 8 == 0 and 16-B "
             "alignment");
  OT_REQUIRE(!p.rowpart || plane, "ot_mixed_gemm_rms: OT_EPI_ROW_RSTD with N = %d > %d needs the plane GEMM "
             "(split mode, a pre-split B image, 16-B aligned A)", N, GT);
  // the row maxima are written by the split-mode plane GEMM's vector epilogue only (the edge kernels' scalar
  // epilogue has no row reduction): refuse a call that would leave them unwritten
  OT_REQUIRE(!p.rowmax_out || (plane && !one && p.rowmax_n == (int)ceil_div(N, GT)),
             "ot_mixed_gemm_rms: rowmax_out needs the split-mode plane GEMM (pre-split B image, whole tiles, 16-B "
             "aligned A) and rowmax_n == ceil(N / %d) = %d (got %d)", GT, (int)ceil_div(N, GT), p.rowmax_n);
  OT_REQUIRE(!p.a_rowmax || p.a_rowmax_n >= 1, "ot_mixed_gemm_rms: a_rowmax needs a_rowmax_n >= 1");
  // the output bound is taken in the vector epilogue (whole tiles; the edge kernels' scalar epilogue has none)
  OT_REQUIRE(!p.rowabs_out || (!edge && kern != nullptr && p.rowabs_n == (int)ceil_div(N, GT)),
             "ot_mixed_gemm_rms: rowabs_out needs a specialised whole-tile kernel and rowabs_n == ceil(N / %d)", GT);
  OT_REQUIRE(!p.amax_out || (!edge && kern != nullptr),
             "ot_mixed_gemm_rms: amax_out needs a specialised whole-tile kernel (K %% 16 == 0, N %% 128 == 0, 16-B "
             "aligned operands)");
  // (+ K floats of gamma behind the stage buffers for the xn_out side output)
  const size_t xn_lds = p.xn_out ? (size_t)K * 4 : 0;
  const size_t launch_shmem = !plane ? shmem
                              : one ? std::max((size_t)plane_lds + xn_lds, (size_t)(64 * (GT + 4) + 8 * GT) * 4)
                                    : (size_t)plane_lds + xn_lds;
  OT_REQUIRE(kern || !rms_flags, "ot_mixed_gemm_rms: no specialised kernel for epilogue flags %d", epi);
  if (!kern) kern = edge ? mixed_gemm_pick_generic<true>(nt, splt) : mixed_gemm_whole_generic(nt, splt);
  if (wide_lds > 0) {
    const size_t wshm = std::max((size_t)wide_lds + xn_lds, (size_t)(64 * (GT + 4) + 8 * GT) * 4);
    const unsigned wg = wide_kind == 3 ? (unsigned)(ntiles / 2) * (unsigned)(N / PW_COLS)
                                       : (unsigned)ntiles * (unsigned)(N / (wide_kind == 2 ? PB_COLS : PW_COLS));
    hipLaunchKernelGGL(kern, dim3(wg), dim3(wide_kind == 3 ? 512 : 256), wshm, s, p);
  } else if (p.panel_w > 0) {
    const unsigned npan = (unsigned)((p.ntn + p.panel_w - 1) / p.panel_w);
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles * npan), dim3(256), (size_t)panel_lds, s, p);
    plane_panel_launched();
  } else {
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), launch_shmem, s, p);
  }
  OT_LAUNCH_CHECK("ot_mixed_gemm");
  if (dgpart) {
    launch_colsum_reduce(dgpart, ntiles, N, rms->dgamma, rms->accumulate_dgamma, s, dgpart + (int64_t)ntiles * N);
    OT_LAUNCH_CHECK("ot_mixed_gemm_rms(dgamma)");
  }
  if (p.rowpart) {
    const int64_t nr = (int64_t)ntiles * GT;
    hipLaunchKernelGGL(row_rstd_finish_kernel, dim3(ceil_div(nr, 256)), dim3(256), 0, s, p.rowpart, p.ntn, out_rows,
                       nr, N, rms->eps, rms->rstd_out);
    OT_LAUNCH_CHECK("ot_mixed_gemm_rms(rstd)");
  }
  return OT_OK;
}

extern "C" int ot_mixed_gemm(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                             int a_xform, const float* a_rstd, const float* a_gamma,
                             const float* W, int64_t w_gstride, int64_t ldw, int N,
                             const int32_t* tile_group, int ntiles,
                             const float* bias, int64_t bias_gstride,
                             float* C, int64_t ldc, const int32_t* out_rows, int epi,
                             const float* res, int64_t ldres, int res_tok,
                             const float* aux, int64_t ldaux,
                             uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                             const int32_t* tail_pos, int precision, void* stream) {
  return mixed_gemm_impl(mode, A, lda, K, in_rows, a_xform, a_rstd, a_gamma, W, w_gstride, ldw, N, tile_group,
                         ntiles, bias, bias_gstride, C, ldc, out_rows, epi, res, ldres, res_tok, aux, ldaux, seed,
                         site, drop_rate, tail_K, tail_I, tail_pos, nullptr, nullptr, 0, 0, precision, stream);
}

extern "C" int ot_mixed_gemm_img(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                                 int a_xform, const float* a_rstd, const float* a_gamma,
                                 const float* W, int64_t w_gstride, int64_t ldw, int N,
                                 const int32_t* tile_group, int ntiles,
                                 const float* bias, int64_t bias_gstride,
                                 float* C, int64_t ldc, const int32_t* out_rows, int epi,
                                 const float* res, int64_t ldres, int res_tok,
                                 const float* aux, int64_t ldaux,
                                 uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                                 const int32_t* tail_pos, const uint16_t* b_image, int image_ntn, int image_tn0,
                                 int precision, void* stream) {
  return mixed_gemm_impl(mode, A, lda, K, in_rows, a_xform, a_rstd, a_gamma, W, w_gstride, ldw, N, tile_group,
                         ntiles, bias, bias_gstride, C, ldc, out_rows, epi, res, ldres, res_tok, aux, ldaux, seed,
                         site, drop_rate, tail_K, tail_I, tail_pos, nullptr, b_image, image_ntn, image_tn0, precision, stream);
}

extern "C" size_t ot_mixed_gemm_rms_workspace_size(int ntiles, int N) {
  const int64_t parts = ntiles > 0 ? ntiles : 1;
  return (size_t)(parts * N + colsum_scratch_floats(parts, N)) * sizeof(float);
}

extern "C" int ot_mixed_gemm_rms(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                                 int a_xform, const float* a_rstd, const float* a_gamma,
                                 const float* W, int64_t w_gstride, int64_t ldw, int N,
                                 const int32_t* tile_group, int ntiles,
                                 const float* bias, int64_t bias_gstride,
                                 float* C, int64_t ldc, const int32_t* out_rows, int epi,
                                 const float* res, int64_t ldres, int res_tok,
                                 const float* aux, int64_t ldaux,
                                 uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                                 const int32_t* tail_pos, const ot_rms_epilogue* rms, int precision, void* stream) {
  OT_REQUIRE(rms, "ot_mixed_gemm_rms: null epilogue operands");
  OT_REQUIRE(rms->struct_size == sizeof(ot_rms_epilogue),
             "ot_mixed_gemm_rms: ot_rms_epilogue.struct_size %zu != %zu (header of another ot_version)",
             rms->struct_size, sizeof(ot_rms_epilogue));
  return mixed_gemm_impl(mode, A, lda, K, in_rows, a_xform, a_rstd, a_gamma, W, w_gstride, ldw, N, tile_group,
                         ntiles, bias, bias_gstride, C, ldc, out_rows, epi, res, ldres, res_tok, aux, ldaux, seed,
                         site, drop_rate, tail_K, tail_I, tail_pos, rms, nullptr, 0, 0, precision, stream);
}

extern "C" int ot_mixed_gemm_rms_img(int mode, const float* A, int64_t lda, int K, const int32_t* in_rows,
                                     int a_xform, const float* a_rstd, const float* a_gamma,
                                     const float* W, int64_t w_gstride, int64_t ldw, int N,
                                     const int32_t* tile_group, int ntiles,
                                     const float* bias, int64_t bias_gstride,
                                     float* C, int64_t ldc, const int32_t* out_rows, int epi,
                                     const float* res, int64_t ldres, int res_tok,
                                     const float* aux, int64_t ldaux,
                                     uint32_t seed, uint32_t site, float drop_rate, int tail_K, int tail_I,
                                     const int32_t* tail_pos, const ot_rms_epilogue* rms, const uint16_t* b_image,
                                     int image_ntn, int image_tn0, int precision, void* stream) {
  OT_REQUIRE(rms, "ot_mixed_gemm_rms: null epilogue operands");
  OT_REQUIRE(rms->struct_size == sizeof(ot_rms_epilogue),
             "ot_mixed_gemm_rms: ot_rms_epilogue.struct_size %zu != %zu (header of another ot_version)",
             rms->struct_size, sizeof(ot_rms_epilogue));
  return mixed_gemm_impl(mode, A, lda, K, in_rows, a_xform, a_rstd, a_gamma, W, w_gstride, ldw, N, tile_group,
                         ntiles, bias, bias_gstride, C, ldc, out_rows, epi, res, ldres, res_tok, aux, ldaux, seed,
                         site, drop_rate, tail_K, tail_I, tail_pos, rms, b_image, image_ntn, image_tn0, precision, stream);
}
