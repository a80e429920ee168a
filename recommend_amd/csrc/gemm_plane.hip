// The 128 x 128 plane GEMMs of ot_mixed_gemm*_img (dispatch: mixed_gemm_impl, gemm.hip): plane_gemm_kernel and the
// panel form of its pair arithmetic, plane_panel_kernel, with their process-wide switches.
#include <atomic>

#include "gemm.h"

namespace ot {

#ifndef OT_PLANE_BF16_NSTG         // stage buffers of the bf16-mode plane GEMM (3: 4 workgroups / CU)
#define OT_PLANE_BF16_NSTG 3
#endif
constexpr int PLANE_BF16_NSTG = OT_PLANE_BF16_NSTG;

// Plane GEMM (split-bf16, NT): the B operand (a weight bank) arrives pre-split — ot_split_images
// writes, once per optimizer step, every 128-column x 16-k block of B as its three bf16 planes in
// the exact LDS image the MFMA fragments read ([plane][128 n][2 halves of 8 k], the halves of rows
// with bit 3 of n set swapped: conflict-free ds_read_b128) — and the A operand (activations, f32)
// is copied global -> LDS unchanged.  Both move by global_load_lds_dwordx4 (no VGPR staging, no
// LDS store instructions), three stages deep, one raw barrier per 16-k stage with a counted
// vmcnt.  Waves are 4x1: wave w owns rows 32w..32w+31 x all 128 columns, so each A element is
// read and split into its planes exactly once per tile, right before its MFMAs (the A image rows
// are 64 B with the 16-B chunk swizzle c ^ ((r >> 2) & 3): conflict-free ds_read_b128).  An
// RMSNorm prologue is folded into B (gamma scales B's k rows when the image is built) and its row
// factor rstd is applied in the epilogue; a GELU prologue runs on the fragment before the split.
constexpr int PG_A_BYTES = GT * 16 * 4;            // A stage image: 128 rows x 16 f32 (B's: PG_B_BYTES, gemm.h)
constexpr int PG_STG_BYTES = PG_A_BYTES + PG_B_BYTES;
static_assert(64 * (GT + 4) * 4 + 8 * GT * 4 <= 2 * PG_STG_BYTES, "plane GEMM epilogue LDS");
// TERMS 2 row metadata (128 output rows + 128 row factors): behind the epilogue tile and its dgamma slots, inside
// the second stage's third-plane KiBs that the two-plane copies never write
constexpr int PG_META_OFF = 64 * (GT + 4) * 4 + 8 * GT * 4;
constexpr int PG_META_BYTES = 2 * GT * 4;
static_assert(PG_META_OFF >= PG_STG_BYTES + PG_A_BYTES + 2 * GT * 16 * 2 && PG_META_OFF + PG_META_BYTES <= 2 * PG_STG_BYTES,
              "plane GEMM row metadata LDS");

// TERMS = 6: split mode (three planes, six products); TERMS = 1: OT_MATMUL_BF16 (plane 0 of the image
// holds the weight rounded to nearest, A is rounded at fragment time, one product; only plane 0 is
// copied, so a stage is 12 KiB instead of 20 KiB)
template <int TERMS>
constexpr int pg_stage_bytes() { return PG_A_BYTES + (TERMS == 1 ? GT * 16 * 2 : PG_B_BYTES); }

// TERMS = 2 (split mode with the RMSNorm prologue): the scaled fp16 pair, three f16 products.  B's image is the pair
// of B[k][n] s_n (ot_split_images: every gamma-folded image, s_n from the column max); A = x gets one power-of-two
// scale per row from the bound |x_k| <= sqrt(K) / rstd (sum_k x_k^2 = K (1 / rstd^2 - eps)) — no pass over the row;
// the accumulator is unscaled per row and column before the epilogue.  Precision: 22 bits relative to the bound
// (a row whose largest |x| is 2^-b of it keeps 22 - b bits there).
template <int AXT, int EPIT, int NSTG, int MINW, int TERMS = 6>
__global__ __launch_bounds__(256, MINW) void plane_gemm_kernel(GemmArgs p) {
  static_assert(NSTG >= 2 && NSTG <= 4, "plane GEMM stages");
  static_assert(TERMS == 6 || TERMS == 1 || (TERMS == 2 && (AXT == OT_AX_RMSNORM || AXT == OT_AX_GELU || AXT == OT_AX_NONE)),
                "plane GEMM terms");
  // OT_AX_BF16: A holds bf16 values (the FFN1 epilogue's stored gelu(U)): 32 B per row and stage, the
  // lane's fragment is one 16-B LDS read, no conversion (bf16 mode only)
  // OT_AX_BF16_RMSNORM: bf16 x with the RMSNorm applied as the RMSNorm prologue does on this kernel (gamma
  // folded into the B image, rstd as the epilogue's row scale)
  constexpr bool ABF = AXT == OT_AX_BF16 || AXT == OT_AX_BF16_RMSNORM;
  constexpr bool RSC = AXT == OT_AX_RMSNORM || AXT == OT_AX_BF16_RMSNORM;
  static_assert(!ABF || TERMS == 1, "bf16 A operands go with OT_MATMUL_BF16");
  constexpr int STG = pg_stage_bytes<TERMS>();
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int nwg = p.ntm * p.ntn;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tm = wg / p.ntn, tn = wg % p.ntn;
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const int n0 = tn * GT;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int nk = p.K >> 4;

  // glds sources.  A: wave w's instruction i fills LDS bytes [(2w+i) KiB, +1 KiB) of the A image =
  // rows 16(2w+i) .. +15, lane j -> row + j/4, physical chunk j%4 = logical chunk (j%4) ^ swizzle.
  // Rows of the tile past the row map (in_rows < 0) read row 0: their outputs are never stored.
  const float* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (2 * wave + i) * 16 + (lane >> 2);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    const int lc = (lane & 3) ^ ((r >> 2) & 3);
    asrc[i] = p.A + (int64_t)ir * p.lda + 4 * lc;
  }
  // bf16 A: one instruction per wave = rows 32w .. +31, lane j -> row + j/2, physical 16-B half j%2 =
  // logical half (j%2) ^ ((row >> 3) & 1) (rows li and li + 8 of a fragment read then hit other banks)
  const char* asrcb;
  {
    const int r = 32 * wave + (lane >> 1);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    asrcb = reinterpret_cast<const char*>(p.A) + ((int64_t)ir * p.lda + 8 * ((lane & 1) ^ ((r >> 3) & 1))) * 2;
  }
  // B: the (g, tile) image is nk consecutive 12-KiB stage blocks; wave w copies KiB 3w .. 3w+2 (a
  // weight shared by every group, w_gstride 0 like Wo, has one group's image)
  const int gb = p.w_gstride ? g : 0;
  const char* bimg0 = reinterpret_cast<const char*>(p.bimg) + ((int64_t)gb * p.bimg_ntn + p.bimg_tn0 + tn) * nk * PG_B_BYTES;
  constexpr int BPL = TERMS == 2 ? 2 : 3;              // B planes copied per stage (split modes)
  const char* bsrc = bimg0 + (BPL * wave) * 1024 + 16 * lane;
  const char* bsrc1 = bimg0 + wave * 1024 + 16 * lane;

  auto issue = [&](int ks, int buf) {
    char* sb = lds + buf * STG;
    if (ABF) {
      __builtin_amdgcn_global_load_lds((const void*)(asrcb + 32 * ks), (lds_void_t*)(sb + wave * 1024), 16, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + 16 * ks), (lds_void_t*)(sb + (2 * wave + i) * 1024),
                                         16, 0, 0);
    }
    if (TERMS == 1) {                                 // plane 0 only: wave w copies its KiB w
      __builtin_amdgcn_global_load_lds((const void*)(bsrc1 + (int64_t)ks * PG_B_BYTES),
                                       (lds_void_t*)(sb + PG_A_BYTES + wave * 1024), 16, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < BPL; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(bsrc + (int64_t)ks * PG_B_BYTES + i * 1024),
                                         (lds_void_t*)(sb + PG_A_BYTES + (BPL * wave + i) * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  const int ra = 32 * wave + li;                      // this lane's A row (fragment row li)
  const int aoff0 = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
  const int aoff1 = ra * 64 + 16 * ((2 * h + 1) ^ ((li >> 2) & 3));
  const int boff = PG_A_BYTES + li * 32 + 16 * (h ^ ((li >> 3) & 1));
  const int aoffb = ra * 32 + 16 * (h ^ ((li >> 3) & 1));  // bf16 A

  // normalised-A side output (AXT == OT_AX_RMSNORM, first column tile): this lane's fragment row ra; gamma
  // is copied to LDS behind the stage buffers first (a global load in the loop would make the compiler
  // wait for every outstanding stage copy)
  bool xnw = false;
  float xrs = 0.f;
  uint16_t* xnp = nullptr;
  float* gsm = reinterpret_cast<float*>(lds + NSTG * STG);
  constexpr bool XN = RSC && TERMS == 1;             // (bf16 mode only: split-mode registers are full)
  if (XN && p.xn_out && tn == 0) {
    for (int k = 4 * t; k < p.K; k += 4 * 256)
      *reinterpret_cast<f32x4*>(gsm + k) = *reinterpret_cast<const f32x4*>(p.a_gamma + k);
    const int64_t xgr = (int64_t)tm * GT + ra;
    const int xir = p.in_rows ? p.in_rows[xgr] : (int)xgr;
    xnw = xir >= 0;
    if (xnw) {
      xrs = p.a_rstd[xir];
      xnp = p.xn_out + (int64_t)xir * p.ldxn + 8 * h;
    }
  }

  // TERMS 2: this lane's A row scale from the RMSNorm bound sqrt(K) / rstd (the row's rstd, as the epilogue reads
  // it; loaded ahead of the stage copies, so waiting for it does not drain them)
  // (GELU prologue: the row's bound max(max_j a_rowmax, 0.17) >= max |gelu(a)|, from the producer's partial maxima)
  float abound = 1.f;
  // (not with the GELU prologue: those instantiations sit at the register cap, and their epilogue reads only the
  // output rows — independent loads, no dependent chain to remove)
  constexpr bool PMETA = TERMS == 2 && AXT != OT_AX_GELU;
  int mrow = 0;                                       // row metadata of fragment row ra (TERMS 2, p.rowmeta)
  bool mok = false;
  if constexpr (TERMS == 2) {
    const int64_t gr = (int64_t)tm * GT + ra;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    mok = ir >= 0;
    if (PMETA && p.rowmeta) mrow = p.out_rows ? p.out_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    if constexpr (AXT == OT_AX_RMSNORM) {
      abound = p.a_rstd[ir];
    } else {
      // GELU prologue: signed maxima of u, floored at 0.17 >= |gelu| of negative u; plain A: the rows' max |a| parts
      abound = AXT == OT_AX_GELU ? 0.17f : 0.f;
      for (int j = 0; j < p.a_rowmax_n; ++j) abound = fmaxf(abound, p.a_rowmax[(int64_t)ir * p.a_rowmax_n + j]);
    }
  }
  issue(0, 0);
  if (NSTG >= 3 && nk > 1) issue(1, 1);
  if (NSTG >= 4 && nk > 2) issue(2, 2);
  float asc = 1.f, ainv = 1.f;
  const int* rmeta = nullptr;
  if constexpr (TERMS == 2) {
    asc = pow2_scale14(AXT == OT_AX_RMSNORM ? sqrtf((float)p.K) / abound : abound);
    ainv = 1.f / asc;
    // row metadata for the epilogue, one lane per tile row (the lanes of half 0: row ra), parked where neither the
    // two-plane stage copies nor the epilogue tile reach; the row factor is the rstd this lane holds as abound.
    // The main loop's barriers (lgkmcnt(0) before each) publish it long before the epilogue reads.
    if (PMETA && p.rowmeta) {
      int* rm = reinterpret_cast<int*>(lds + PG_META_OFF);
      if (h == 0) {
        rm[ra] = mrow;
        if (RSC) rm[GT + ra] = __float_as_int(mok ? abound : 0.f);
      }
      rmeta = rm;
    }
  }
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's copies of stage kt are done (with 3 stages the 5 (TERMS 1: 3) of stage kt+1 may
    // still fly), every wave's after the barrier; the barrier also retires every read of the buffer
    // that the copies of stage kt+NSTG-1 then overwrite (last read in iteration kt-1)
    constexpr int OPS = ABF ? 2 : (TERMS == 1 ? 3 : 2 + BPL);    // copies per wave and stage
    const int ahead = (NSTG - 2 < nk - 1 - kt) ? NSTG - 2 : nk - 1 - kt;   // later stages that may still fly
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * OPS) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(OPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + NSTG - 1 < nk) issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
    const char* sb = lds + (kt % NSTG) * STG;
    u32x4 fb[4][3];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int q = 0; q < (TERMS == 1 ? 1 : BPL); ++q)
        fb[nb][q] = *reinterpret_cast<const u32x4*>(sb + boff + q * 4096 + nb * 1024);
    if constexpr (ABF) {
      u32x4 fa[3];
      fa[0] = *reinterpret_cast<const u32x4*>(sb + aoffb);
      if (XN && xnw) {                                  // from the bf16 x: (x * gamma) * rstd, rounded
        const float* gp = gsm + 16 * kt + 8 * h;
        const u32x4 w = fa[0];
        const f32x4 a0 = {__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                          __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
        const f32x4 a1 = {__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u),
                          __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
        const f32x4 v0 = a0 * *reinterpret_cast<const f32x4*>(gp) * xrs;
        const f32x4 v1 = a1 * *reinterpret_cast<const f32x4*>(gp + 4) * xrs;
        const u32x2 b0 = bf16_rne4(v0), b1 = bf16_rne4(v1);
        *reinterpret_cast<u32x4*>(xnp + 16 * kt) = u32x4{b0.x, b0.y, b1.x, b1.y};
      }
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma_bf16(fa[0], fb[nb][0], acc[nb]);
      continue;
    }
    f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0);
    f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + aoff1);
    if (XN && xnw) {                                    // k = 16 kt + 8 h .. + 7: (a * gamma) * rstd, rounded
      const float* gp = gsm + 16 * kt + 8 * h;
      const f32x4 v0 = a0 * *reinterpret_cast<const f32x4*>(gp) * xrs;
      const f32x4 v1 = a1 * *reinterpret_cast<const f32x4*>(gp + 4) * xrs;
      const u32x2 b0 = bf16_rne4(v0), b1 = bf16_rne4(v1);
      *reinterpret_cast<u32x4*>(xnp + 16 * kt) = u32x4{b0.x, b0.y, b1.x, b1.y};
    }
    if (AXT == OT_AX_GELU) {
      // scalar form here (bit-identical per element to gelu_erf4): the packed pairs measured 2-3% slower in this
      // main loop (register pressure next to the stage copies), while the epilogues and the weight gradient gain
      a0.x = gelu_erf(a0.x); a0.y = gelu_erf(a0.y); a0.z = gelu_erf(a0.z); a0.w = gelu_erf(a0.w);
      a1.x = gelu_erf(a1.x); a1.y = gelu_erf(a1.y); a1.z = gelu_erf(a1.z); a1.w = gelu_erf(a1.w);
    }
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    u32x4 fa[3];
    if constexpr (TERMS == 2) {
      pair8(av, asc, fa);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma_pair(fa, fb[nb], acc[nb]);
    } else {
      split8t<TERMS == 1 ? 1 : 6>(av, fa);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma_terms<TERMS == 1 ? 1 : 6>(fa, fb[nb], acc[nb]);
    }
  }
  if constexpr (TERMS == 2) {
    // unscale: row factor 1 / s_a (held by the lane whose A row it is: lane = row within the wave), column
    // factor 1 / s_b (ot_split_images' column scales, plane 2 of the tile's first unit); exact powers of two
    const float* csc = reinterpret_cast<const float*>(bimg0 + 2 * GT * 16 * 2);
    const float bad = reinterpret_cast<const uint32_t*>(csc)[GT] == PAIR_IMAGE_TAG ? 1.f : __builtin_nanf("");
    float cinv[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) cinv[nb] = bad / csc[32 * nb + li];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ri = __shfl(ainv, (r & 3) + 8 * (r >> 2) + 4 * h, 64);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb][r] *= ri * cinv[nb];
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                    // the epilogue reuses the stage buffers
  gemm_vec_epilogue<EPIT, 1, RSC, MINW >= 4 ? OT_PLANE_EPI_RBN : 8, TERMS == 1>(p, acc, smem, tm, n0, g, 0, -1, rmeta);
}

// Panel form of the pair plane GEMM (TERMS 2, launches with two or more column tiles): one workgroup owns a row tile
// and walks `panel_w` of its column tiles.  The row maps, the A source addresses, the A row scale and the epilogue's
// row metadata are formed once per row tile; a tile's first two stages are copied while the tile before it runs its
// epilogue.  For that the epilogue keeps out of the stage ring: each wave moves its own 32 rows through a private
// 8- or 2-row LDS slice in 4 or 16 passes (no workgroup barrier in the epilogue, so nothing drains the copies in flight).
// One barrier after a tile's last k-step frees the ring for the next tile's first stages.  Every wait on the copies
// is vmcnt(0) (the two-stage ring waits for all of a stage anyway; at a tile's first k-step that also covers the
// epilogue stores issued since).  Per output: the same MFMA chain in the same k order, the same unscale and the same
// epilogue arithmetic as plane_gemm_kernel — bit-identical results.  Measured (profiles/r07/README.md) it does not
// beat plane_gemm_kernel with the row metadata in LDS, in any variant below: never selected by default.
constexpr int PP_STG = PG_A_BYTES + 2 * GT * 16 * 2;           // A stage + the pair's two B planes (16 KiB)
constexpr int PP_CLD = GT + 4;
constexpr int PP_EPI_OFF = 2 * PP_STG;
// SR = rows of one wave's epilogue slice: 8 (50,688 B: three workgroups per CU) or 2 (38,016 B: four)
constexpr int pp_epi_wave(int SR) { return SR * PP_CLD * 4; }
constexpr int pp_meta_off(int SR) { return PP_EPI_OFF + 4 * pp_epi_wave(SR); }
constexpr int pp_lds(int SR) { return pp_meta_off(SR) + PG_META_BYTES; }
static_assert(3 * pp_lds(8) <= 160 * 1024 && 4 * pp_lds(2) <= 160 * 1024, "panel plane GEMM LDS");

// the epilogue of one wave's 32 x 128 block (acc[nb][r]: row (r & 3) + 8 (r >> 2) + 4 h, column 32 nb + li): per pass
// the wave parks 8 rows in its slice, then each half-wave finishes 4 of them, a float4 column chunk per lane — the
// lane-to-column layout of gemm_vec_epilogue (the row reductions run over the same 32 lanes in the same order)
template <int EPIT, bool ROWSCALE, int SR>
__device__ __forceinline__ void panel_epilogue(const GemmArgs& p, const f32x16* acc, float* ctw, const int* rmeta,
                                               int row0, int n0, f32x4 bias4, float& am) {
  static_assert(!(EPIT & ~(OT_EPI_BIAS | OT_EPI_GELU_BWD | OT_EPI_ROWDOT)), "panel plane GEMM epilogue flags");
  constexpr int epi = EPIT;
  constexpr bool ROWDOT = (EPIT & OT_EPI_ROWDOT) != 0;
  const int lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const int c4 = li, col = n0 + 4 * c4;
  const f32x4 rdb4 = bias4;                          // OT_EPI_ROWDOT: the bias subtracted from aux
  // a pass parks HQ accumulator registers per lane: slice row q + HQ h' holds register HQ j + q of half h'; the
  // half-wave h then finishes slice rows h + 2 i
  constexpr int HQ = SR / 2;
  static_assert(SR == 8 || SR == 2, "panel epilogue slice rows");
#pragma unroll
  for (int j = 0; j < 16 / HQ; ++j) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int q = 0; q < HQ; ++q) ctw[(q + HQ * h) * PP_CLD + 32 * nb + li] = acc[nb][HQ * j + q];
    int orow[HQ];
    float rsc[HQ];
#pragma unroll
    for (int i = 0; i < HQ; ++i) {
      const int sr = h + 2 * i, r = HQ * j + sr % HQ;
      const int tr = row0 + (r & 3) + 8 * (r >> 2) + 4 * (sr / HQ);
      orow[i] = rmeta[tr];
      if (ROWSCALE) rsc[i] = __int_as_float(rmeta[GT + tr]);
    }
    f32x4 aux4[HQ];
#pragma unroll
    for (int i = 0; i < HQ; ++i) {
      const int64_t o = orow[i] < 0 ? 0 : orow[i];
      if (epi & OT_EPI_GELU_BWD) aux4[i] = *reinterpret_cast<const f32x4*>(p.aux + o * p.ldaux + col);
    }
    // the slice's writes before its reads (LDS runs a wave's accesses in order; this keeps the compiler's order too)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < HQ; ++i) {
      const int orr = orow[i];
      f32x4 v = *reinterpret_cast<const f32x4*>(ctw + (h + 2 * i) * PP_CLD + 4 * c4);
      if (ROWSCALE) v = v * rsc[i];
      if (epi & OT_EPI_BIAS) v += bias4;
      if (p.rowmax_out) {                                  // this tile's largest C of the row (signed)
        float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
        mx = row32_max(mx);
        if (orr >= 0 && c4 == 0) p.rowmax_out[(int64_t)orr * p.rowmax_n + n0 / GT] = mx;
      }
      if (epi & OT_EPI_GELU_BWD) {
        v *= gelu_erf_grad4(aux4[i]);
        if (p.gelu_out && orr >= 0) {                      // the stored GELU (W2 weight gradient's A)
          const f32x4 hv = gelu_erf4(aux4[i]);
          store_out4_bf16(p.gelu_out + (int64_t)orr * p.ldgelu + col, hv);
        }
        if (ROWDOT) {                                      // this tile's part of sum_f dU_f (U_f - b_f)
          const f32x4 ub = aux4[i] - rdb4;
          const float sd = row32_sum(v.x * ub.x + v.y * ub.y + v.z * ub.z + v.w * ub.w);
          if (orr >= 0 && c4 == 0) p.rowdot[(int64_t)orr * p.rowdot_n + n0 / GT] = sd;
        }
      }
      if (orr >= 0) store_out4(p.C + (int64_t)orr * p.ldc + col, v);
      if (orr >= 0) am = amax4(am, v);
      if (p.rowabs_out) {                                  // this tile's max |C| of the row (fp16-pair consumer)
        float mx = amax4(0.f, v);
        mx = row32_max(mx);
        if (orr >= 0 && c4 == 0) p.rowabs_out[(int64_t)orr * p.rowabs_n + n0 / GT] = mx;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the slice is rewritten by the next pass
  }
}

// MINW / SR: workgroups per CU and the epilogue slice rows that fit (3 / 8, 4 / 2).  HOLDA (K = 128 only, two
// workgroups per CU): the row tile's A pair fragments are formed on its first column tile and held in registers (64
// VGPRs) for the others, which copy only B.
template <int AXT, int EPIT, int MINW = 3, int SR = 8, bool HOLDA = false>
__global__ __launch_bounds__(256, MINW) void plane_panel_kernel(GemmArgs p) {
  static_assert(AXT == OT_AX_RMSNORM || AXT == OT_AX_NONE, "panel plane GEMM prologues");
  static_assert(MINW * pp_lds(SR) <= 160 * 1024, "panel plane GEMM LDS per CU");
  constexpr bool RSC = AXT == OT_AX_RMSNORM;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  const int pw = p.panel_w, npan = (p.ntn + pw - 1) / pw;
  const int wg = xcd_remap(blockIdx.x, p.ntm * npan);
  const int tm = wg / npan, tnb = (wg % npan) * pw;
  const int tne = tnb + pw < p.ntn ? tnb + pw : p.ntn;
  const int g = p.tile_group ? p.tile_group[tm] : 0;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 5, li = lane & 31;
  const int nk = p.K >> 4;

  // stage copies as plane_gemm_kernel's (A: wave w's instruction i fills KiB 2w + i of the A image; B: KiB 2w + i of
  // the two planes); column tile tn's image is nk consecutive 12-KiB blocks
  const float* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (2 * wave + i) * 16 + (lane >> 2);
    const int64_t gr = (int64_t)tm * GT + r;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    const int lc = (lane & 3) ^ ((r >> 2) & 3);
    asrc[i] = p.A + (int64_t)ir * p.lda + 4 * lc;
  }
  const int gb = p.w_gstride ? g : 0;
  const int64_t tstride = (int64_t)nk * PG_B_BYTES;
  const char* bpan = reinterpret_cast<const char*>(p.bimg) + ((int64_t)gb * p.bimg_ntn + p.bimg_tn0) * tstride;
  const int blane = 2 * wave * 1024 + 16 * lane;
  auto issue = [&](int tn, int ks, int buf) {
    char* sb = lds + buf * PP_STG;
    const char* bs = bpan + tn * tstride + (int64_t)ks * PG_B_BYTES + blane;
    if (!HOLDA || tn == tnb) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + 16 * ks), (lds_void_t*)(sb + (2 * wave + i) * 1024),
                                         16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(bs + i * 1024),
                                       (lds_void_t*)(sb + PG_A_BYTES + (2 * wave + i) * 1024), 16, 0, 0);
  };

  const int ra = 32 * wave + li;                      // this lane's A row (fragment row li)
  const int aoff0 = ra * 64 + 16 * ((2 * h) ^ ((li >> 2) & 3));
  const int aoff1 = ra * 64 + 16 * ((2 * h + 1) ^ ((li >> 2) & 3));
  const int boff = PG_A_BYTES + li * 32 + 16 * (h ^ ((li >> 3) & 1));

  // the row's bound, output row and row factor, once per row tile (plane_gemm_kernel: abound, p.rowmeta)
  float abound;
  int mrow;
  bool mok;
  {
    const int64_t gr = (int64_t)tm * GT + ra;
    int ir = p.in_rows ? p.in_rows[gr] : (int)gr;
    mok = ir >= 0;
    mrow = p.out_rows ? p.out_rows[gr] : (int)gr;
    ir = ir < 0 ? 0 : ir;
    if constexpr (AXT == OT_AX_RMSNORM) {
      abound = p.a_rstd[ir];
    } else {
      abound = 0.f;
      for (int j = 0; j < p.a_rowmax_n; ++j) abound = fmaxf(abound, p.a_rowmax[(int64_t)ir * p.a_rowmax_n + j]);
    }
  }
  issue(tnb, 0, 0);
  if (nk > 1) issue(tnb, 1, 1);
  const float asc = pow2_scale14(AXT == OT_AX_RMSNORM ? sqrtf((float)p.K) / abound : abound);
  const float ainv = 1.f / asc;
  int* rmeta = reinterpret_cast<int*>(lds + pp_meta_off(SR));
  if (h == 0) {
    rmeta[ra] = mrow;
    if (RSC) rmeta[GT + ra] = __float_as_int(mok ? abound : 0.f);
  }
  float* ctw = reinterpret_cast<float*>(lds + PP_EPI_OFF + wave * pp_epi_wave(SR));
  float am = 0.f;
  u32x4 fah[HOLDA ? 8 : 1][2];

  for (int tn = tnb; tn < tne; ++tn) {
    // this tile's column scales and form tag (plane 2 of its first unit), back long before the unscale
    const float* csc = reinterpret_cast<const float*>(bpan + tn * tstride + 2 * GT * 16 * 2);
    float craw[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) craw[nb] = csc[32 * nb + li];
    uint32_t tag = reinterpret_cast<const uint32_t*>(csc)[GT];
    // (and its bias chunk: a load inside the epilogue would wait for the next tile's copies issued before it)
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (EPIT & (OT_EPI_BIAS | OT_EPI_ROWDOT))
      bias4 = *reinterpret_cast<const f32x4*>(p.bias + (int64_t)g * p.bias_gstride + tn * GT + 4 * li);
    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    auto kstep = [&](int kt) {
      // stage kt has landed (every wave's after the barrier); the barrier also retires iteration kt - 1's reads of
      // the buffer that stage kt + 1 then overwrites (stages 0 and 1 were copied ahead of the tile)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kt >= 1 && kt + 1 < nk) issue(tn, kt + 1, (kt + 1) & 1);
      const char* sb = lds + (kt & 1) * PP_STG;
      u32x4 fb[4][3];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int q = 0; q < 2; ++q) fb[nb][q] = *reinterpret_cast<const u32x4*>(sb + boff + q * 4096 + nb * 1024);
      u32x4 fa[3];
      if (!HOLDA || tn == tnb) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(sb + aoff0);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(sb + aoff1);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        pair8(av, asc, fa);
        if (HOLDA) { fah[kt][0] = fa[0]; fah[kt][1] = fa[1]; }
      } else {
        fa[0] = fah[kt][0]; fa[1] = fah[kt][1];
      }
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma_pair(fa, fb[nb], acc[nb]);
    };
    if constexpr (HOLDA) {                             // (nk == 8: the held fragments are indexed at compile time)
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) kstep(kt);
    } else {
      for (int kt = 0; kt < nk; ++kt) kstep(kt);
    }
    // the scales, the tag and the bias are waited for here, with no copy in flight: the empty statement reads their
    // registers, so the compiler's wait for those loads stands above it and cannot sink below the next tile's copies
    // (where it would be a vmcnt(0) that drains them before the epilogue starts)
    asm volatile("" : "+v"(craw[0]), "+v"(craw[1]), "+v"(craw[2]), "+v"(craw[3]), "+v"(tag), "+v"(bias4));
    {
      const float bad = tag == PAIR_IMAGE_TAG ? 1.f : __builtin_nanf("");
      float cinv[4];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) cinv[nb] = bad / craw[nb];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float ri = __shfl(ainv, (r & 3) + 8 * (r >> 2) + 4 * h, 64);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb][r] *= ri * cinv[nb];
      }
    }
    if (tn + 1 < tne) {                                // every wave is past its last stage reads: the ring is free
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      issue(tn + 1, 0, 0);
      if (nk > 1) issue(tn + 1, 1, 1);
    }
    panel_epilogue<EPIT, RSC, SR>(p, acc, ctw, rmeta, 32 * wave, tn * GT, bias4, am);
  }
  if (p.amax_out) amax_flush(p.amax_out, am);            // (uniform: every wave reaches it)
}

// The pair plane GEMM's epilogue row metadata (output rows, RMSNorm row factors): 1 = loaded once per tile by one
// lane per row and parked in LDS (default), 0 = read from the row maps per epilogue row batch; the same values
#ifndef OT_PLANE_ROWMETA
#define OT_PLANE_ROWMETA 1
#endif
static std::atomic<int> g_plane_rowmeta{OT_PLANE_ROWMETA};
extern "C" int ot_plane_rowmeta(int on) {
  const int old = g_plane_rowmeta.load(std::memory_order_relaxed);
  if (on >= 0) g_plane_rowmeta.store(on ? 1 : 0, std::memory_order_relaxed);
  return old;
}

// The panel form of the pair plane GEMM (plane_panel_kernel): 0 = off (default: measured, it does not beat the
// one-tile kernel with the row metadata in LDS, profiles/r07/README.md), 1 = auto (the pair launches with two or more
// column tiles whose prologue / epilogue it has; the width by plane_panel_width, which keeps small launches on the
// one-tile kernel), w in 2 .. 64 = on with w column tiles per workgroup (tests, A/B), 100 + w = the same on the
// four-workgroups-per-CU variant, 200 + w = on the held-A variant (K = 128; other K: the default variant);
// bit-identical outputs either way
#ifndef OT_PLANE_PANEL
#define OT_PLANE_PANEL 0
#endif
static std::atomic<int> g_plane_panel{OT_PLANE_PANEL};
extern "C" int ot_plane_panel(int on) {
  const int old = g_plane_panel.load(std::memory_order_relaxed);
  if (on >= 0) g_plane_panel.store(on > 299 ? 299 : on, std::memory_order_relaxed);
  return old;
}
// launches that took the panel form since the library was loaded (tests: which kernel a launch ran on)
static std::atomic<long long> g_plane_panel_launches{0};
extern "C" int ot_plane_panel_launches(void) {
  return (int)(g_plane_panel_launches.load(std::memory_order_relaxed) & 0x7fffffff);
}
void plane_panel_launched() { g_plane_panel_launches.fetch_add(1, std::memory_order_relaxed); }
// variant 0: three workgroups per CU (8-row epilogue slices); 1: four (2-row slices); 2: two, A fragments held
void (*plane_panel_for(int x, int e, int variant, int* lds))(GemmArgs) {
  *lds = pp_lds(variant == 1 ? 2 : 8);
#define OT_PANEL_PICK(AX_, EP_)                                                                          \
  if (x == (AX_) && e == (EP_))                                                                          \
    return variant == 2 ? plane_panel_kernel<AX_, EP_, 2, 8, true>                                       \
         : variant == 1 ? plane_panel_kernel<AX_, EP_, 4, 2, false> : plane_panel_kernel<AX_, EP_, 3, 8, false>;
  OT_PANEL_PICK(OT_AX_RMSNORM, 0)
  OT_PANEL_PICK(OT_AX_RMSNORM, OT_EPI_BIAS)
  OT_PANEL_PICK(OT_AX_NONE, OT_EPI_GELU_BWD)
  OT_PANEL_PICK(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_ROWDOT)
#undef OT_PANEL_PICK
  return nullptr;
}
// Column tiles per workgroup.  The grid is ntiles x ceil(ntn / width) workgroups on 3 per CU; the last round of
// resident workgroups may be nearly empty, so the width is halved while the grid has fewer than four rounds (the tail
// is then at most a quarter of the launch; C2's 4,480 row tiles on 768 slots keep the whole width: 5.8 rounds).
// 0 (the one-tile kernel) when even two tiles per workgroup leave less than one round of workgroups: a small launch
// would run its tiles one after another on a few CUs while the others stand idle.
int plane_panel_width(int ntiles, int ntn) {
  static const int slots = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return 3 * cus;
  }();
  int w = ntn;
  while (w > 2 && (int64_t)ntiles * ((ntn + w - 1) / w) < 4 * (int64_t)slots) w = (w + 1) / 2;
  if ((int64_t)ntiles * ((ntn + w - 1) / w) < slots) return 0;
  return w;
}

// plane_gemm_kernel's (a_xform, epi) pairs.  OT_PLANE_LIST: every mode (bf16 mode: one product; split mode: six
// products, or the fp16 pair with the RMSNorm prologue or A's row maxima); OT_PLANE_BF16_LIST: the bf16 mode only
#define OT_PLANE_LIST(X)                                                                       \
  X(OT_AX_RMSNORM, 0)                                                                          \
  X(OT_AX_RMSNORM, OT_EPI_BIAS)                                                                \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT)                                \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL)                                                 \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)              \
  X(OT_AX_GELU, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                               \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_DROPOUT)                                              \
  X(OT_AX_NONE, OT_EPI_RESIDUAL)                                                               \
  X(OT_AX_NONE, OT_EPI_BIAS)                                                                   \
  X(OT_AX_NONE, OT_EPI_GELU_BWD)                                                               \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_ROWDOT)                                               \
  X(OT_AX_NONE, 0)                                                                             \
  X(OT_AX_NONE, OT_EPI_ACCUMULATE)                                                             \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)                            \
  X(OT_AX_NONE, OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                                             \
  X(OT_AX_NONE, OT_EPI_RMSNORM_BWD)                                                            \
  X(OT_AX_NONE, OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT)
#define OT_PLANE_BF16_LIST(X)                                                                  \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16)                               \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_C_BF16)                                               \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16 | OT_EPI_AUX_BF16)             \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_C_BF16 | OT_EPI_AUX_BF16)                             \
  X(OT_AX_NONE, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_AUX_BF16)                             \
  X(OT_AX_RMSNORM, OT_EPI_BIAS | OT_EPI_C_BF16)                                                \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT)                                \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL)                                                 \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_DROPOUT | OT_EPI_ROW_RSTD)              \
  X(OT_AX_BF16, OT_EPI_BIAS | OT_EPI_RESIDUAL | OT_EPI_ROW_RSTD)                               \
  X(OT_AX_BF16, OT_EPI_RMSNORM_BWD)                                                            \
  X(OT_AX_BF16, OT_EPI_RMSNORM_BWD | OT_EPI_DROPOUT)                                           \
  X(OT_AX_BF16, 0)                                                                             \
  X(OT_AX_BF16, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16 | OT_EPI_AUX_BF16)             \
  X(OT_AX_BF16, OT_EPI_GELU_BWD | OT_EPI_ROWDOT | OT_EPI_C_BF16)                               \
  X(OT_AX_BF16_RMSNORM, 0)                                                                     \
  X(OT_AX_BF16_RMSNORM, OT_EPI_BIAS)                                                           \
  X(OT_AX_BF16_RMSNORM, OT_EPI_BIAS | OT_EPI_C_BF16)

// plane_gemm_kernel for (a_xform, epi), or null; its stage LDS bytes in *stage_lds (under 64 KiB: no opt-in)
void (*plane_gemm_for(int x, int e, bool one, bool rowmax, int* stage_lds))(GemmArgs) {
  *stage_lds = one ? PLANE_BF16_NSTG * pg_stage_bytes<1>() : 2 * PG_STG_BYTES;
#define OT_PLANE_PICK(AX_, EP_)                                                                \
  if (x == (AX_) && e == (EP_))                                                                \
    return one ? plane_gemm_kernel<AX_, EP_, PLANE_BF16_NSTG, 4, 1>                            \
         : rowmax ? plane_gemm_kernel<AX_, EP_, 2, 4, 2>                                       \
                  : plane_gemm_kernel<AX_, EP_, 2, 4, (AX_) == OT_AX_RMSNORM ? 2 : 6>;
  OT_PLANE_LIST(OT_PLANE_PICK)
#undef OT_PLANE_PICK
#define OT_PLANE_PICK(AX_, EP_) \
  if (one && x == (AX_) && e == (EP_)) return plane_gemm_kernel<AX_, EP_, PLANE_BF16_NSTG, 4, 1>;
  OT_PLANE_BF16_LIST(OT_PLANE_PICK)
#undef OT_PLANE_PICK
  return nullptr;
}

}  // namespace ot
