"""The transformer block of OneTransModel (reference OneTransBlock.call, model.py:186-200): its forward, recompute
and backward launches (``_block_forward``, ``_Block``, ``_fold_backward``), the per-forward fp16-pair bounds
(``PairBounds``, ``a_row_bounds``) and the two form functions that decide, once per call, which launch runs and which
side outputs it writes (``block_fwd_form`` / ``block_bwd_form``, as ``attn_fwd_route`` / ``attn_bwd_route`` do for the
attention kernels).  The launching code reads only the fields of those records."""

from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import kernels as K
from ._lib import (OT_AX_BF16, OT_AX_BF16_RMSNORM, OT_AX_GELU, OT_AX_RMSNORM, OT_EPI_AUX_BF16, OT_EPI_BIAS,
                   OT_EPI_C_BF16, OT_EPI_DROPOUT, OT_EPI_GELU_BWD, OT_EPI_RESIDUAL, OT_EPI_RMSNORM_BWD,
                   OT_EPI_ROW_RSTD, OT_EPI_ROWDOT, OT_GEMM_NT, OT_WG_D_BF16)
from .layout import TILE

RMS_EPS = 1e-6   # RMSNorm eps, model.py:14


def layer_seed(seed: int, b0: int, I: int, d: int) -> int:
    """Dropout seed of a layer whose local sample b is global sample b0 + b.  The mask hashes the 32-bit
    element index (b*I + p)*d + n as idx * 0x9E3779B1 + seed (common.h drop_keep), so shifting every
    index by b0*I*d is the same as adding b0*I*d*0x9E3779B1 to the seed (mod 2^32): the kernels keep
    local indices and the masks equal the full batch's (oracle dropout_scale's ``b0``)."""
    return (seed + b0 * I * d * 0x9E3779B1) & 0xFFFFFFFF if b0 else seed


def _layer_valid(kvalid, I):
    """The slice of layer 0's key-padding mask [B, L0] that a layer of I tokens reads under the tail keep: its last I
    columns, as (tensor, element offset, row stride) — the same array, no copy."""
    L0 = kvalid.shape[1]
    return kvalid, L0 - I, L0


def _attn_qpos(cfg, pos):
    """Kept-query positions for the attention kernels: None (the tail rule, I - K + j) when the keep is
    the reference's tail — ot_pyramid_select returns exactly that set there, in order."""
    return None if getattr(cfg, 'pyramid_select', 'tail') == 'tail' else pos


class PairBounds:
    """Magnitude bounds of the fp16-pair weight gradients' operands (split mode, ot_mixed_gemm_wgrad_ex) for one
    forward and its backward: a zeroed float per layer and slot, into which the producing kernel folds max |output|
    (an atomic max: the recompute's second fold of the same values changes nothing).  ``out`` is the producer's
    view; ``get`` the consumer's, None unless a producer took it — no bound, like no object: the exact split."""
    SLOTS = ('o', 'u', 'dy2', 'du', 'dyo', 'dqkv', 'dx')   # |O|, |U|, |dY2|, |dU|, |dX1 masked|, |dQKV|, |dX|

    def __init__(self, layers: int, device):
        self.t, self._taken = torch.zeros(layers, 8, device=device), {}
        self._dx = {}

    def put_dx(self, l: int, dx: torch.Tensor, rowabs: torch.Tensor) -> None:
        """Block ``l``'s input gradient with the row maxima (and, in slot 'dx', the bound) its QKV dgrad reported:
        block ``l - 1`` masks this tensor inside its fused FFN backward (``ffn_bwd_rule``)."""
        self._dx[l] = (dx, dx._version, rowabs)

    def take_dx(self, l: int, dx2: torch.Tensor):
        """(row maxima, bound) of ``dx2`` if it is the tensor block ``l`` reported, unchanged since; else None."""
        e = self._dx.pop(l, None)
        if (e is None or e[0].data_ptr() != dx2.data_ptr() or e[0].shape != dx2.shape or e[1] != dx2._version
                or not dx2.is_contiguous()):
            return None
        return e[2], self.get(l, 'dx')

    @classmethod
    def begin(cls, layers: int, device, mode: str, pair_wgrad: bool) -> Optional['PairBounds']:
        """For a forward in split mode with ONETRANS_PAIR_WGRAD on that a backward can follow; else None."""
        return cls(layers, device) if mode == 'split' and pair_wgrad and torch.is_grad_enabled() else None

    def out(self, l: int, name: str) -> torch.Tensor:
        return self._taken.setdefault((l, name), self.t[l, self.SLOTS.index(name):][:1])

    def get(self, l: int, name: str) -> Optional[torch.Tensor]:
        return self._taken.get((l, name))


def a_row_bounds(on: bool, x, ld: int, rows: int, n: int, reported=None) -> Dict:
    """The GEMM arguments that hand an fp16-pair image (``on``: gemm_pair) its A rows' maxima: those x's producer
    ``reported``, else one row-absmax pass over x [rows, n]."""
    if on and reported is None:
        reported = torch.empty(rows, (n + 255) // 256, device=x.device)
        K.rows_absmax(x, ld, rows, n, reported)
    return dict(a_rowmax=reported, a_rowmax_n=reported.shape[1]) if on else {}


# =============================================================================== forms
class BlockSaved(NamedTuple):
    """What a block's forward keeps for its backward.  qkv: float32, or the fp8 forward's bf16 dequantised copy; u: the
    FFN pre-activation (bf16 under ``FwdForm.u_bf``; None when no backward reads it); h: the stored bf16 gelu(u);
    xn1 / x1n: the bf16 normalised QKV / FFN1 inputs; yf: the folded attention's probability-weighted raw rows
    [B, H, d].  Each of the last four is None where its ``FwdForm`` field is off."""
    x: torch.Tensor
    rstd1: torch.Tensor
    qkv: torch.Tensor
    o: torch.Tensor
    lse: torch.Tensor
    x1: torch.Tensor
    rstd2: torch.Tensor
    u: Optional[torch.Tensor]
    h: Optional[torch.Tensor]
    xn1: Optional[torch.Tensor]
    x1n: Optional[torch.Tensor]
    yf: Optional[torch.Tensor]


class FwdForm(NamedTuple):
    """Which launches one block forward makes and which side outputs they write (``block_fwd_form``)."""
    fuse: bool         # the Wo / FFN2 epilogues emit the rstd of the rows they finish (OT_EPI_ROW_RSTD, fuse_with)
    take_x16: bool     # ask for the bf16 copy of x the previous block's FFN2 epilogue stored (take_x16)
    xn: bool           # the QKV GEMM also stores its normalised A rows in bf16 (saved xn1)
    x1n: bool          # ... and the FFN1 GEMM its own (saved x1n)
    fold: Optional[Tuple[int, int]]   # the folded one-query attention's dedicated key range (fold_gate), or None
    qpos: bool         # the attention kernels get the kept-query positions (a keep other than the tail)
    qkv16: bool        # fp8 training: the dequantised operands go to a bf16 copy that replaces qkv
    pair_wo: bool      # Wo's forward image is in the pair form: the GEMM needs O's row maxima
    o_rep: bool        # the attention forward reports |O| and O's row maxima
    x1_16: bool        # the Wo epilogue stores a bf16 copy of x1 for FFN1's A
    h: bool            # the FFN1 epilogue stores h = gelu(u) in bf16 (saved h)
    u_bf: bool         # ... and u itself in bf16
    pair_w2: bool      # W2's forward image is in the pair form: FFN1 writes u's row maxima and |U|
    ffn_fused: bool    # FFN1 -> GELU -> FFN2 in one launch (ot_ffn_fused_fwd)
    write_u: bool      # that launch writes u
    x2_16: bool        # the FFN2 epilogue stores a bf16 copy of x2 for the next block (put_x16)
    fused2: bool       # the norm2 backward in the FFN dgrad epilogues at d > 128 (rowdot partials)


def block_fwd_form(m, l: int, I: int, Kq: int, training: bool, select: bool, masked: bool, need_out: bool = True,
                   need_u: bool = True) -> FwdForm:
    """The form of block ``l``'s forward on I tokens keeping Kq, from the model's state, the matmul mode and the
    K.* switches as they are now.  ``masked``: a key-padding mask is given; ``need_out`` False: the backward's
    recompute, which stops after FFN1; ``need_u`` False: no backward will read this call's u."""
    cfg = m.config
    d, f, hd = cfg.hidden_dim, cfg.ffn_dim, cfg.hidden_dim // cfg.num_heads
    mode = K.matmul_mode()
    wqkv, wo, w1, w2 = (f'blk.{l}.{w}' for w in ('wqkv', 'wo', 'w1', 'w2'))
    img1, img2 = m.bimg(w1) is not None, m.bimg(w2) is not None
    fuse = m.fuse_with((wo, 'fwd'), (w2, 'fwd'))
    # the last layer's one query, folded through the shared K / V projection (ot_attn_fold_*)
    fold = m.fold_gate(I, Kq, select, masked)
    qpos = select and getattr(cfg, 'pyramid_select', 'tail') != 'tail'
    qp = qpos or None                          # (the capability queries ask only whether positions are given)
    # bf16 mode, training: the QKV / FFN1 GEMMs also store their normalised A rows in bf16 (ot_rms_epilogue
    # .xn_out) for the copy-staged bf16 weight gradients of Wqkv / W1 (operands read once, no norm re-applied)
    xn = training and mode == 'bf16' and d % TILE == 0 and m.bimg(wqkv) is not None
    # the bf16 residual copy feeds FFN1 only as an OT_AX_BF16_RMSNORM operand, which needs W1's plane image
    x1_16 = fuse and m.x16_on(d) and img1
    # bf16 mode: the FFN1 epilogue also stores h = gelu(u) rounded to bf16 — exactly the operand the bf16
    # FFN2 GEMM would form at fragment time — so FFN2 reads 2 B per element and evaluates no erf (it did,
    # once per output column tile), and the W2 weight gradient reuses h
    h = mode == 'bf16' and img2 and img1 and f % TILE == 0
    fused2 = m.fuse_bwd2 and not m.fuse_bwd and f % TILE == 0
    # split mode: the FFN1 epilogue also writes each column tile's row maximum of u, from which the FFN2 plane GEMM
    # takes its rows' fp16-pair scales (its W2 image is in the pair form, layout kscale -2)
    # (exactly when W2's forward image is in the pair form, layout.pair_images: then W1's forward image exists, f % 128
    # == 0, and the FFN1 plane GEMM writes every row's maxima; the library refuses rowmax_out anywhere else and a
    # pair image read without them multiplies NaN into the output)
    pair_w2 = mode == 'split' and img2 and (w2, 'fwd') in m.layout.pair_images
    assert not pair_w2 or (not h and img1 and f % TILE == 0), \
        'the pair-form W2 image needs the FFN1 plane GEMM to write the row maxima of u'
    # split mode, d == 128, the block output wanted: FFN1 -> GELU -> FFN2 in one launch (ot_ffn_fused_fwd: u stays in
    # the accumulators, no row maxima round trip); the recompute (need_out False) wants u only: the FFN1 launch
    ffn_fused = bool(pair_w2 and need_out and d == TILE and f <= K.FFN_FUSED_MAX_F and not x1_16 and K.ffn_fused())
    return FwdForm(
        fuse=fuse, take_x16=d % TILE == 0 and need_out, xn=xn, x1n=xn and h, fold=fold, qpos=qpos,
        # with the key-grouped bf16 backward (the backward rounds the operands to bf16 anyway)
        qkv16=bool(m.attn_fp8 and training and K.attn_bwd_bf16_supported(I, Kq, hd, qp)),
        pair_wo=m.gemm_pair(wo, 'fwd'),
        # (the masked attention reports no bounds: O's row maxima then come from a_row_bounds' own pass, and the Wo
        # weight gradient, without |O|, runs the exact split; nor does the folded attention: its B rows go through the
        # row-absmax pass and the exact-split Wo gradient)
        o_rep=not masked and not m.attn_fp8 and fold is None and K.attn_amax_supported(I, Kq, hd, qp),
        x1_16=x1_16, h=h,
        # u in bf16 (as a bf16 Keras policy stores it): its one reader is then the FFN2 dgrad's GELU' / row-dot
        # epilogue (OT_EPI_AUX_BF16), which needs the fused norm2 backward's bf16-dU form
        u_bf=h and fused2, pair_w2=pair_w2, ffn_fused=ffn_fused, write_u=need_u or not ffn_fused,
        x2_16=fuse and m.x16_on(d) and img2, fused2=fused2)


def ffn_bwd_rule(m, l: int, rate: float, has_bounds: bool, masked: bool) -> Tuple[bool, bool]:
    """(fused, mask) for block ``l``'s FFN backward.  fused: ot_ffn_fused_bwd's form applies — split mode, d == 128,
    pair-form W2 / W1 dgrad images, the norm2 backward in the FFN1 dgrad's epilogue, ONETRANS_FFN_FUSED_BWD /
    K.ffn_fused_bwd_on on: both input gradients in one launch.  mask: ... and under dropout it masks dx2 inside that
    launch and inside the W2 weight gradient (no dropout pass, no dY2): with the pair weight gradients'
    bounds, no padding mask, and ONETRANS_BWD_MASK_FUSED / K.bwd_mask_fused on.  Block ``l`` asks this of itself,
    and block ``l + 1`` asks it of block ``l`` to know whether its QKV dgrad must report dx's row maxima."""
    d, f = m.config.hidden_dim, m.config.ffn_dim
    fused = bool(l >= 0 and m.fuse_bwd and d == TILE and f % TILE == 0 and f <= K.FFN_FUSED_MAX_F
                 and m.dgrad_pair(f'blk.{l}.w2') and m.dgrad_pair(f'blk.{l}.w1') and K.ffn_fused_bwd_on())
    return fused, bool(fused and rate > 0 and has_bounds and not masked and K.bwd_mask_fused())


class BwdForm(NamedTuple):
    """Which launches one block backward makes and which side outputs they write (``block_bwd_form``)."""
    du_bf: bool        # dU (and dY2) in bf16: the FFN2 dgrad epilogue stores it so (OT_EPI_C_BF16)
    pw2: bool          # the W2 / W1 / Wo / Wqkv dgrad images are in the pair form: their GEMMs need the A rows' maxima
    pw1: bool
    pwo: bool
    pqkv: bool
    ffn_bwd: bool      # both FFN input gradients in one launch (ot_ffn_fused_bwd)
    mask_fused: bool   # ... which masks dx2 itself, as does the W2 weight gradient (keep bits)
    dy2_bound: bool    # the dropout pass reports |dY2|
    dy2_rowmax: bool   # ... and dY2's row maxima
    hbf: bool          # the FFN2 dgrad epilogue stores gelu(U) in bf16 for the W2 weight gradient
    du_bound: bool     # the FFN2 dgrad reports |dU|
    du_rowmax: bool    # ... and dU's row maxima
    dx1_ep: bool       # FFN1 dgrad -> norm2 backward in the epilogue, which reports on dyo
    a1n: bool          # the W1 weight gradient reads the bf16 x1n (both operands bf16: copy-staged)
    dq_bf: bool        # dQKV in bf16 (OT_ATTN_DQKV_BF16)
    dq_rep: bool       # the attention backward reports |dQKV|
    an1: bool          # the Wqkv weight gradient reads the bf16 xn1
    qkv_ep: bool       # QKV dgrad -> norm1 backward in the epilogue
    rep_dx: bool       # ... which reports dx's row maxima and bound: the block below masks dx itself


def block_bwd_form(m, l: int, I: int, Kq: int, rate: float, masked: bool, has_bounds: bool, u_bound: bool,
                   fwd: FwdForm) -> BwdForm:
    """The form of block ``l``'s backward, from the model's state, the matmul mode and the K.* switches as they are
    now and ``fwd``, the form of the forward (or recompute) that wrote the saved activations.  ``has_bounds``: a
    PairBounds goes with this forward; ``u_bound``: its |U| slot was taken."""
    cfg = m.config
    d, f, hd = cfg.hidden_dim, cfg.ffn_dim, cfg.hidden_dim // cfg.num_heads
    mode = K.matmul_mode()
    qp = fwd.qpos or None
    fused2 = fwd.fused2
    du_bf = fused2 and fwd.h and m.bimg(f'blk.{l}.w1', 'dgrad') is not None
    pw2, pw1, pwo, pqkv = (m.dgrad_pair(f'blk.{l}.{w}') for w in ('w2', 'w1', 'wo', 'wqkv'))
    fused, mask = ffn_bwd_rule(m, l, rate, has_bounds, masked)
    # (float32 dU: dU is written for the W1 weight gradient but not read back, and its row maxima stay in registers)
    ffn_bwd = fused and not du_bf and not fwd.h
    # dx2's row maxima and bound come from its producer, the QKV dgrad of the block above, else from one row-absmax pass
    mask_fused = ffn_bwd and u_bound and mask
    dy2_rep = rate > 0 and not du_bf           # the float32 dropout reports |dY2|, and row maxima at some widths
    # does the FFN2 dgrad report dU's bound and row maxima?  (its whole-tile vector epilogue does)
    du_rep = fused2 or (((has_bounds and not du_bf) or pw2 or pw1) and f % TILE == 0)
    # bf16 mode, key-grouped backward (C5): dQKV in bf16 (OT_ATTN_DQKV_BF16) — the QKV dgrad (bf16 A) and
    # the Wqkv weight gradient (OT_WG_D_BF16) round it to bf16 anyway: the same values, half the bytes
    dq_bf = bool(mode == 'bf16' and K.attn_bwd_bf16_forms(I, Kq, hd, qp) & _lib.OT_ATTN_DQKV_BF16
                 and m.bimg(f'blk.{l}.wqkv', 'dgrad') is not None)
    dq_rep = not masked and not dq_bf and K.attn_amax_supported(I, Kq, hd, qp, backward=True)
    return BwdForm(
        du_bf=du_bf, pw2=pw2, pw1=pw1, pwo=pwo, pqkv=pqkv, ffn_bwd=ffn_bwd, mask_fused=mask_fused,
        dy2_bound=dy2_rep and not mask_fused,
        dy2_rowmax=bool(dy2_rep and pw2 and K.dropout_rowmax_supported(d) and not mask_fused),
        # bf16 mode with the fused norm2 backward (C5): the FFN2 dgrad epilogue, which reads U for GELU'
        # anyway, also stores gelu(U) in bf16 — the W2 weight gradient then reads 2 B per element instead of
        # U's 4 and evaluates no erf (it did, once per output column tile: 4x at f = 2048, d = 512)
        # (the forward's FFN1 epilogue stored it already under fwd.h)
        hbf=not fwd.h and fused2 and mode == 'bf16',
        du_bound=du_rep and not du_bf, du_rowmax=pw1 and du_rep and not ffn_bwd,
        dx1_ep=bool(m.fuse_bwd or fused2), a1n=fwd.x1n and du_bf, dq_bf=dq_bf, dq_rep=dq_rep, an1=fwd.xn and dq_bf,
        qkv_ep=bool(m.fuse_bwd),
        # (the neighbour is asked with "no padding mask" whatever this block's own mask is: kept as it was; a wrong
        # guess only costs the neighbour its own row-absmax pass, PairBounds.take_dx)
        rep_dx=pqkv and ffn_bwd_rule(m, l - 1, rate, has_bounds, False)[1])


# =============================================================================== launches
def _block_forward(m, l, x, I, Kq, seed, training, form: FwdForm, rstd_in=None, select=False, need_out=True,
                   bounds=None, kvalid=None):
    """The block's forward kernels in the form ``form`` (``_Block.forward``; also the backward's recompute with
    ``need_out=False``, which stops after FFN1: the backward needs u, not the block output).
    ``bounds``: this forward's PairBounds or None.
    ``kvalid``: layer 0's key-padding mask [B, L0] (uint8; seq_padding_mask) or None; the layer reads its last I
    columns.
    Returns (x2, rstd_out, saved, pos, inv, rate); saved: a BlockSaved."""
    cfg = m.config
    d, f, H = cfg.hidden_dim, cfg.ffn_dim, cfg.num_heads
    hd = d // H
    B = x.shape[0] // I
    dev = x.device
    maps = m.maps(B, I, Kq)
    ma, mt = maps['all'].to(dev), maps['tail'].to(dev)
    na, nt = maps['all'].ntiles, maps['tail'].ntiles
    rate = cfg.dropout_rate if training else 0.0
    dflag = OT_EPI_DROPOUT if rate > 0 else 0
    wqkv, wo = m.pT(f'blk.{l}.wqkv'), m.pT(f'blk.{l}.wo')          # transposed shadow: [G][N][K]
    w1, b1, w2, b2 = m.pT(f'blk.{l}.w1'), m.p(f'blk.{l}.b1'), m.pT(f'blk.{l}.w2'), m.p(f'blk.{l}.b2')
    g1, g2 = m.p(f'blk.{l}.norm1'), m.p(f'blk.{l}.norm2')
    iqkv, iw1, w2img = m.bimg(f'blk.{l}.wqkv'), m.bimg(f'blk.{l}.w1'), m.bimg(f'blk.{l}.w2')
    # norm1 -> rstd only; the QKV GEMM applies it in its A prologue
    if rstd_in is not None and rstd_in.numel() == B * I:
        rstd1 = rstd_in
    else:
        rstd1 = torch.empty(B * I, device=dev)
        K.rmsnorm_fwd(x, d, B * I, d, rstd1, eps=RMS_EPS)
    # pyramid keep (model.py:287-302, 371): the kept query positions come from the wavefront
    # top-K select (ot_pyramid_select); with no score (reference semantics) they are the tail
    qrows, pos, inv = mt['rows'][0], None, None
    if select:
        pos = torch.empty(B * Kq, dtype=torch.int32, device=dev)
        inv = torch.empty(B * I, dtype=torch.int32, device=dev)
        if cfg.pyramid_select == 'norm':
            # score = token RMS (1/rstd1): keep the largest; the NS tail is always kept and only the
            # shared-group rows of the tail map change (dedicated_positions='tail', checked in config)
            nf = min(cfg.num_ns_tokens, Kq)
            qrows = qrows.clone()
            K.pyramid_select(B, I, Kq, pos, inv, score=rstd1, sign=-1.0, nforce=nf, map_rows=qrows,
                             map_per_sample=Kq - nf)
        else:
            K.pyramid_select(B, I, Kq, pos, inv)
    tail = (Kq, I, pos)
    # bf16 mode: the block input in bf16 as the previous block's FFN2 epilogue stored it (ot_rms_epilogue
    # .c16_out) — the QKV GEMM reads it (OT_AX_BF16_RMSNORM: the values its fragments would round x to)
    x16 = m.take_x16(l, x) if form.take_x16 else None
    ax1 = OT_AX_BF16_RMSNORM if x16 is not None else OT_AX_RMSNORM
    xa = x16 if x16 is not None else x
    qkv = torch.empty(B * I, 3 * d, device=dev)
    xn1 = torch.empty(B * I, d, dtype=torch.int16, device=dev) if form.xn else None
    x1n = torch.empty(B * Kq, d, dtype=torch.int16, device=dev) if form.x1n else None
    fold, full = form.fold, Kq == I
    if form.xn:
        K.gemm_rms(OT_GEMM_NT, xa, d, d, ma['rows'][0], wqkv if full else (wqkv, d * d), 3 * d * d, d,
                   3 * d if full else 2 * d, ma['tile_group'], na, qkv if full else (qkv, d), 3 * d, ma['rows'][0],
                   epi=0, a_xform=ax1, rstd=rstd1, gamma=g1, m_rows=maps['all'].nrows, device=dev,
                   bimg=iqkv if full else m.bimg(f'blk.{l}.wqkv', tn0=d // TILE), xn_out=xn1, ldxn=d)
    elif full:
        K.gemm(OT_GEMM_NT, xa, d, d, ma['rows'][0], wqkv, 3 * d * d, d, 3 * d, ma['tile_group'], na, qkv,
               3 * d, ma['rows'][0], a_xform=ax1, rstd=rstd1, gamma=g1, m_rows=maps['all'].nrows, bimg=iqkv)
    else:
        # one query and shared-weight keys (fold): K / V of the dedicated rows only (and the query row, which the
        # map holds for the backward) — the attention reads the other keys' raw rows
        mkv, kvm = (maps['fold'].to(dev), maps['fold']) if fold is not None else (ma, maps['all'])
        K.gemm(OT_GEMM_NT, xa, d, d, mkv['rows'][0], (wqkv, d * d), 3 * d * d, d, 2 * d, mkv['tile_group'],
               kvm.ntiles, (qkv, d), 3 * d, mkv['rows'][0], a_xform=ax1, rstd=rstd1, gamma=g1, m_rows=kvm.nrows,
               bimg=m.bimg(f'blk.{l}.wqkv', tn0=d // TILE) if d % TILE == 0 else None)
    if not full:                                     # the kept queries' Q
        K.gemm(OT_GEMM_NT, xa, d, d, qrows, wqkv, 3 * d * d, d, d, mt['tile_group'], nt, qkv,
               3 * d, qrows, a_xform=ax1, rstd=rstd1, gamma=g1, m_rows=maps['tail'].nrows, bimg=iqkv)
    o = torch.empty(B * Kq, d, device=dev)
    lse = torch.empty(B * H * Kq, device=dev)
    # a 'tail' keep (reference rule) is the contiguous tail, which the attention kernels address
    # arithmetically (no per-query position loads; C3 attention 20.2 -> 18.3 ms/step); the select map
    # still drives the GEMM row maps and epilogues
    # fp8 training forward: qkv's operands are replaced by their dequantised fp8 values, so the backward
    # differentiates (nearly) the forward that ran (OT_FP8_DEQUANT; exact for one-term operands, approximate
    # for the default two-term ones: bf16 rounding of hi + lo and the dropped lo.lo product)
    # with the key-grouped bf16 backward, the dequantised operands go to a bf16 copy that replaces qkv as the
    # backward's saved operand (the backward rounds them to bf16 anyway)
    qp_f = _attn_qpos(cfg, pos)
    qkv16 = torch.empty(B * I, 3 * d, dtype=torch.int16, device=dev) if form.qkv16 else None
    out = (lambda name: bounds.out(l, name)) if bounds is not None else (lambda name: None)
    # the Wo forward on the fp16 pair (pair-form Wo image): O's row maxima, per head, and |O| from the slice forward
    rm_o = torch.empty(B * Kq, H, device=dev) if form.pair_wo and form.o_rep else None
    yf = None
    if fold is not None:
        yf = torch.empty(B * H, d, device=dev)
        K.attn_fold_fwd(x, d, rstd1, g1, m.p(f'blk.{l}.wqkv'), 3 * d, wqkv, d, qkv, 3 * d, B, H, I, hd, fold, o, lse,
                        yf)
    elif kvalid is not None:
        K.attn_fwd_masked(qkv, 3 * d, B, H, I, Kq, hd, o, lse, _layer_valid(kvalid, I), qpos=qp_f)
    else:
        K.attn_fwd(qkv, 3 * d, B, H, I, Kq, hd, o, lse, qpos=qp_f, fp8=m.attn_fp8, dequant=m.attn_fp8 and training,
                   fp8_terms=m.fp8_terms, deq16=qkv16, amax=out('o') if form.o_rep else None, rowmax=rm_o)
    pa_o = a_row_bounds(form.pair_wo, o, d, B * Kq, d, rm_o)
    if qkv16 is not None:
        qkv = qkv16
    # x1 = x[tail] + drop(o @ Wo)      (model.py:117, 193)
    x1 = torch.empty(B * Kq, d, device=dev)
    rstd2 = torch.empty(B * Kq, device=dev)
    x1_16 = torch.empty(B * Kq, d, dtype=torch.int16, device=dev) if form.x1_16 else None
    if form.fuse:
        K.gemm_rms(OT_GEMM_NT, o, d, d, mt['rows'][1], wo, 0, d, d, mt['tile_group'], nt, x1, d, mt['rows'][1],
                   epi=OT_EPI_RESIDUAL | dflag | OT_EPI_ROW_RSTD, res=x, ldres=d, res_tok=1, seed=seed,
                   site=2 * l, drop=rate, tail=tail, m_rows=maps['tail'].nrows, rstd_out=rstd2, eps=RMS_EPS,
                   bimg=m.bimg(f'blk.{l}.wo'), c16_out=x1_16, ldc16=d, device=dev, **pa_o)
    else:
        K.gemm_rms(OT_GEMM_NT, o, d, d, mt['rows'][1], wo, 0, d, d, mt['tile_group'], nt, x1, d, mt['rows'][1],
                   epi=OT_EPI_RESIDUAL | dflag, res=x, ldres=d, res_tok=1, seed=seed, site=2 * l, drop=rate,
                   tail=tail, m_rows=maps['tail'].nrows, bimg=m.bimg(f'blk.{l}.wo'), device=dev, **pa_o)
        K.rmsnorm_fwd(x1, d, B * Kq, d, rstd2, eps=RMS_EPS)
    # u = norm2(x1) @ W1[g] + b1[g]  (pre-activation; GELU applied by its consumers)
    h = torch.empty(B * Kq, f, dtype=torch.int16, device=dev) if form.h else None
    u = (torch.empty(B * Kq, f, device=dev, dtype=torch.int16 if form.u_bf else torch.float32)
         if form.write_u else None)
    if form.ffn_fused:
        x2 = torch.empty(B * Kq, d, device=dev)
        rstd_out = torch.empty(B * Kq, device=dev) if form.fuse else None
        K.ffn_fused_fwd(x1, d, mt['rows'][1], mt['tile_group'], nt, rstd2, iw1[0],
                        m.layout.images[(f'blk.{l}.w1', 'fwd')][1], w2img[0],
                        m.layout.images[(f'blk.{l}.w2', 'fwd')][1], b1, f, b2, d, f, x2, d, u_out=u, ldu=f,
                        u_amax=out('u'), rstd_out=rstd_out, eps=RMS_EPS, seed=seed, site=2 * l + 1, drop=rate,
                        tail=tail, m_rows=maps['tail'].nrows)
        return x2, rstd_out, BlockSaved(x, rstd1, qkv, o, lse, x1, rstd2, u, None, xn1, None, yf), pos, inv, rate
    umax = torch.empty(B * Kq, f // TILE, device=dev) if form.pair_w2 else None
    a1, ax_1 = (x1, OT_AX_RMSNORM) if x1_16 is None else (x1_16, OT_AX_BF16_RMSNORM)
    if h is not None:
        K.gemm_rms(OT_GEMM_NT, a1, d, d, mt['rows'][1], w1, d * f, d, f, mt['tile_group'], nt, u, f, mt['rows'][1],
                   a_xform=ax_1, rstd=rstd2, gamma=g2, bias=b1, bias_gstride=f,
                   epi=OT_EPI_BIAS | (OT_EPI_C_BF16 if form.u_bf else 0), m_rows=maps['tail'].nrows, bimg=iw1,
                   gelu_out=h, ldgelu=f, xn_out=x1n, ldxn=d)
    elif umax is not None:
        K.gemm_rms(OT_GEMM_NT, a1, d, d, mt['rows'][1], w1, d * f, d, f, mt['tile_group'], nt, u, f, mt['rows'][1],
                   a_xform=ax_1, rstd=rstd2, gamma=g2, bias=b1, bias_gstride=f, epi=OT_EPI_BIAS,
                   m_rows=maps['tail'].nrows, bimg=iw1, rowmax_out=umax, rowmax_n=umax.shape[1],
                   amax_out=out('u'))                 # |U| >= |gelu(U)|: the W2 wgrad's A bound
    else:
        K.gemm(OT_GEMM_NT, a1, d, d, mt['rows'][1], w1, d * f, d, f, mt['tile_group'], nt, u, f, mt['rows'][1],
               a_xform=ax_1, rstd=rstd2, gamma=g2, bias=b1, bias_gstride=f, epi=OT_EPI_BIAS,
               m_rows=maps['tail'].nrows, bimg=iw1)
    saved = BlockSaved(x, rstd1, qkv, o, lse, x1, rstd2, u, h, xn1, x1n, yf)
    if not need_out:
        return None, None, saved, pos, inv, rate
    # x2 = x1 + drop(gelu(u) @ W2[g] + b2[g])     (model.py:154-161, 198)
    x2 = torch.empty(B * Kq, d, device=dev)
    rstd_out = None
    a2, ax2 = (h, OT_AX_BF16) if h is not None else (u, OT_AX_GELU)
    pa_u = a_row_bounds(form.pair_w2, u, f, B * Kq, f, umax)
    if form.fuse:
        rstd_out = torch.empty(B * Kq, device=dev)
        x2_16 = torch.empty(B * Kq, d, dtype=torch.int16, device=dev) if form.x2_16 else None
        K.gemm_rms(OT_GEMM_NT, a2, f, f, mt['rows'][1], w2, f * d, f, d, mt['tile_group'], nt, x2, d,
                   mt['rows'][1], a_xform=ax2, bias=b2, bias_gstride=d,
                   epi=OT_EPI_BIAS | OT_EPI_RESIDUAL | dflag | OT_EPI_ROW_RSTD, res=x1, ldres=d, res_tok=0,
                   seed=seed, site=2 * l + 1, drop=rate, tail=tail, m_rows=maps['tail'].nrows,
                   rstd_out=rstd_out, eps=RMS_EPS, bimg=w2img, c16_out=x2_16, ldc16=d, **pa_u)
        m.put_x16(l + 1, x2, x2_16)
    elif umax is not None:
        K.gemm_rms(OT_GEMM_NT, a2, f, f, mt['rows'][1], w2, f * d, f, d, mt['tile_group'], nt, x2, d, mt['rows'][1],
                   a_xform=ax2, bias=b2, bias_gstride=d, epi=OT_EPI_BIAS | OT_EPI_RESIDUAL | dflag, res=x1,
                   ldres=d, res_tok=0, seed=seed, site=2 * l + 1, drop=rate, tail=tail,
                   m_rows=maps['tail'].nrows, bimg=w2img, **pa_u)
    else:
        K.gemm(OT_GEMM_NT, a2, f, f, mt['rows'][1], w2, f * d, f, d, mt['tile_group'], nt, x2, d, mt['rows'][1],
               a_xform=ax2, bias=b2, bias_gstride=d, epi=OT_EPI_BIAS | OT_EPI_RESIDUAL | dflag, res=x1,
               ldres=d, res_tok=0, seed=seed, site=2 * l + 1, drop=rate, tail=tail,
               m_rows=maps['tail'].nrows, bimg=w2img)
    return x2, rstd_out, saved, pos, inv, rate


class _Block(torch.autograd.Function):
    """OneTransBlock.call (model.py:186-200) for the last K of I tokens (pyramid / last-layer DCE).
    x: [B*I, d] -> ([B*K, d], rstd of the output rows).

    When d == 128 (one GEMM tile holds whole rows) the RMSNorms are fused into the GEMMs around
    them: the Wo / FFN2 epilogues emit the rstd of the rows they finish (norm2 of this block, norm1
    of the next: ``rstd_in``), and the FFN1 / QKV dgrad epilogues apply the norm backward."""

    @staticmethod
    def forward(ctx, flat, x, m, l, I, Kq, seed, training, rstd_in=None, select=False, bounds=None, kvalid=None):
        # u is read by a backward only: with the recompute (which forms it again) or no input that needs a gradient
        # (inference) this forward need not write it
        form = block_fwd_form(m, l, I, Kq, training, select, kvalid is not None,
                              need_u=not m.recompute and any(ctx.needs_input_grad))
        x2, rstd_out, saved, pos, inv, rate = _block_forward(m, l, x, I, Kq, seed, training, form, rstd_in, select,
                                                             bounds=bounds, kvalid=kvalid)
        if m.recompute:
            # activation recompute: keep the block input (and its rstd); the backward re-runs the
            # forward kernels up to FFN1 (dropout masks and pyramid keeps are deterministic)
            ctx.save_for_backward(saved.x, saved.rstd1)
            ctx.fwd_args = (training, select)
        else:
            ctx.save_for_backward(*saved)
        ctx.m, ctx.l, ctx.I, ctx.Kq, ctx.seed, ctx.rate, ctx.form = m, l, I, Kq, seed, rate, form
        ctx.pos, ctx.inv, ctx.bounds, ctx.kvalid = pos, inv, bounds, kvalid
        if rstd_out is None:
            rstd_out = x2.new_empty(0)          # not fused: the next block computes its own rstd
        ctx.mark_non_differentiable(rstd_out)
        return x2, rstd_out

    @staticmethod
    def backward(ctx, dx2, _drstd=None):
        # the autograd engine runs this on its own thread: enter the model's precision there
        with K.precision(ctx.m.matmul):
            return _Block._backward(ctx, dx2, _drstd)

    @staticmethod
    def _backward(ctx, dx2, _drstd=None):
        m, l, I, Kq, seed, rate, fwd = ctx.m, ctx.l, ctx.I, ctx.Kq, ctx.seed, ctx.rate, ctx.form
        pos, inv, bounds, kvalid = ctx.pos, ctx.inv, ctx.bounds, ctx.kvalid
        if m.recompute:
            xin, rstd_in = ctx.saved_tensors
            training, select = ctx.fwd_args
            fwd = block_fwd_form(m, l, I, Kq, training, select, kvalid is not None, need_out=False)
            _, _, s, pos, inv, _ = _block_forward(m, l, xin, I, Kq, seed, training, fwd, rstd_in, select,
                                                  need_out=False, bounds=bounds, kvalid=kvalid)
        else:
            s = BlockSaved._make(ctx.saved_tensors)
        # fp16-pair weight gradients (split mode): their operands' bounds (PairBounds; None = the exact split runs):
        # |U| and |O| where this backward's own forward took them; ``keep`` goes with the side stream's reads (m.side)
        out = (lambda name: bounds.out(l, name)) if bounds is not None else (lambda name: None)
        b_o, b_u = (bounds.get(l, 'o'), bounds.get(l, 'u')) if bounds is not None else (None, None)
        keep = (bounds.t,) if bounds is not None else ()
        form = block_bwd_form(m, l, I, Kq, rate, kvalid is not None, bounds is not None, b_u is not None, fwd)
        tail = (Kq, I, pos)
        cfg = m.config
        d, f, H = cfg.hidden_dim, cfg.ffn_dim, cfg.num_heads
        hd = d // H
        B = s.x.shape[0] // I
        dev = s.x.device
        acc = m.accumulate_grads
        maps = m.maps(B, I, Kq)
        ma, mt = maps['all'].to(dev), maps['tail'].to(dev)
        na, nt = maps['all'].ntiles, maps['tail'].ntiles
        nca, nct = maps['all'].chunks.shape[0], maps['tail'].chunks.shape[0]
        G = cfg.num_groups
        dx2 = dx2.contiguous()
        rowdot = None
        du_bf, ffn_bwd, mask_fused = form.du_bf, form.ffn_bwd, form.mask_fused
        # FFN branch: dY2 = mask(dx2) — in bf16 with the bf16 dU path (its two readers, the FFN2 dgrad's A and
        # the W2 weight gradient's D, round it to bf16; the latter then runs copy-staged)
        # ... or, with the mask inside the fused FFN backward (ot_ffn_fused_bwd_mask) and inside the W2 weight gradient
        # (OT_WG_D_KEEPBITS, from the keep bits that kernel writes): no dropout pass, dY2 never exists.  dx2's row
        # maxima and bound come from its producer, the QKV dgrad of the block above, else from one row-absmax pass
        dx_rep = bounds.take_dx(l + 1, dx2) if bounds is not None else None
        b_dy2 = out('dy2') if form.dy2_bound else None
        rm_dy2 = torch.empty(B * Kq, (d + 255) // 256, device=dev) if form.dy2_rowmax else None
        dy2 = dx2
        if mask_fused:
            if dx_rep is not None:
                rm_dy2, b_dy2 = dx_rep             # (of dx2: both kernels multiply by 1 / (1 - rate))
            else:
                rm_dy2 = torch.empty(B * Kq, 1, device=dev)
                K.rows_absmax(dx2, d, B * Kq, d, rm_dy2)
                b_dy2 = rm_dy2.max().reshape(1)
            keep_bits = torch.empty(B * Kq, d // 32, dtype=torch.int32, device=dev)
        elif rate > 0:
            dy2 = torch.empty(B * Kq, d, device=dev, dtype=torch.int16 if du_bf else torch.float32)
            K.dropout_apply(dx2, d, dy2, d, B * Kq, d, seed, 2 * l + 1, rate, tail, amax=b_dy2, rowmax=rm_dy2)
        pa2 = a_row_bounds(form.pw2, dy2, d, B * Kq, d, rm_dy2)
        dy_bf = dy2.dtype == torch.int16
        # bf16 mode (C5): dU is stored in bf16 by the FFN2 dgrad epilogue (OT_EPI_C_BF16); its two consumers,
        # the FFN1 dgrad (bf16 A, plane GEMM) and the W1 weight gradient (OT_WG_D_BF16), rounded it to bf16 at
        # fragment / staging time anyway, so only b1's gradient (a column sum of dU) sees the rounding
        du = torch.empty(B * Kq, f, device=dev, dtype=torch.int16 if du_bf else torch.float32)
        cbf = OT_EPI_C_BF16 if du_bf else 0
        hbf = torch.empty(B * Kq, f, dtype=torch.int16, device=dev) if form.hbf else None
        if hbf is None and not mask_fused:
            a2, ax2, b_a2 = (s.h, OT_AX_BF16, None) if fwd.h else (s.u, OT_AX_GELU, b_u)
            with m.side(a2, dy2, *keep):   # weight gradients overlap the dgrad chain (second stream)
                K.wgrad(a2, f, mt['rows'][1], dy2, d, mt['rows'][1], f, d, mt, nct, G,
                        m.g(f'blk.{l}.w2'), f * d, m.g(f'blk.{l}.b2'), d,
                        a_xform=ax2 | (OT_WG_D_BF16 if dy_bf else 0), accumulate=acc, device=dev,
                        m_rows=maps['tail'].nrows, rowmap=maps['tail'], a_bound=b_a2, d_bound=b_dy2)
        b_du = out('du') if form.du_bound else None
        rm_du = torch.empty(B * Kq, f // TILE, device=dev) if form.du_rowmax else None
        rep_du = dict(amax_out=b_du, rowabs_out=rm_du, rowabs_n=f // TILE if rm_du is not None else 0)
        # dx1 and mask(dx1) for the attention branch, with dyo's row maxima and bound where the launch that applies the
        # norm2 backward in its epilogue reports them (a row-wise norm backward reports none)
        dx1 = torch.empty(B * Kq, d, device=dev)
        dyo = torch.empty(B * Kq, d, device=dev) if rate > 0 else dx1
        rm_dyo = torch.empty(B * Kq, (d + TILE - 1) // TILE, device=dev) if form.pwo and form.dx1_ep else None
        b_dyo = out('dyo') if form.dx1_ep else None
        if ffn_bwd:
            # both input gradients in one launch (dU is written for the W1 weight gradient but not read back)
            K.ffn_fused_bwd(dy2, d, pa2['a_rowmax'], pa2['a_rowmax_n'], mt['rows'][1], mt['tile_group'], nt,
                            m.bimg(f'blk.{l}.w2', 'dgrad')[0], m.layout.images[(f'blk.{l}.w2', 'dgrad')][1],
                            m.bimg(f'blk.{l}.w1', 'dgrad')[0], m.layout.images[(f'blk.{l}.w1', 'dgrad')][1], f,
                            s.u, f, du, f, s.x1, d, m.p(f'blk.{l}.norm2'), s.rstd2, dx1, d, m.g(f'blk.{l}.norm2'),
                            du_amax=b_du, dres=dx2, lddres=d, dx_masked=dyo if rate > 0 else None, lddxm=d,
                            accumulate_dgamma=acc, amax_out=b_dyo, rowabs_out=rm_dyo,
                            rowabs_n=1 if rm_dyo is not None else 0, seed=seed, site=2 * l, drop=rate, tail=tail,
                            m_rows=maps['tail'].nrows, device=dev, mask_site=2 * l + 1 if mask_fused else None,
                            keep_out=keep_bits if mask_fused else None, ldkeep=d // 32)
            if mask_fused:
                with m.side(s.u, dx2, keep_bits, b_dy2, *keep):   # after the launch that writes the keep bits
                    K.wgrad(s.u, f, mt['rows'][1], dx2, d, mt['rows'][1], f, d, mt, nct, G, m.g(f'blk.{l}.w2'), f * d,
                            m.g(f'blk.{l}.b2'), d, a_xform=OT_AX_GELU | _lib.OT_WG_D_KEEPBITS, accumulate=acc,
                            device=dev, m_rows=maps['tail'].nrows, rowmap=maps['tail'], a_bound=b_u, d_bound=b_dy2,
                            keep=keep_bits, ldkeep=d // 32, d_scale=1.0 / (1.0 - rate))
        elif fwd.fused2:
            # d > 128: the FFN2 dgrad also emits rowdot[row][f-tile] = sum dU (U - b1) for the norm2 backward
            rowdot = torch.empty(B * Kq, f // TILE, device=dev)
            K.gemm_rms(OT_GEMM_NT, dy2, d, d, mt['rows'][1], m.p(f'blk.{l}.w2'), f * d, d, f, mt['tile_group'], nt,
                       du, f, mt['rows'][1], aux=s.u, ldaux=f, a_xform=OT_AX_BF16 if dy_bf else 0,
                       epi=OT_EPI_GELU_BWD | OT_EPI_ROWDOT | cbf | (OT_EPI_AUX_BF16 if fwd.u_bf else 0),
                       bias=m.p(f'blk.{l}.b1'), bias_gstride=f, rowdot=rowdot, rowdot_n=f // TILE,
                       m_rows=maps['tail'].nrows, device=dev, bimg=m.bimg(f'blk.{l}.w2', 'dgrad'),
                       gelu_out=hbf, ldgelu=f, **rep_du, **pa2)
            if hbf is not None:
                with m.side(hbf, dy2):
                    K.wgrad(hbf, f, mt['rows'][1], dy2, d, mt['rows'][1], f, d, mt, nct, G, m.g(f'blk.{l}.w2'),
                            f * d, m.g(f'blk.{l}.b2'), d, a_xform=OT_AX_BF16, accumulate=acc, device=dev,
                            m_rows=maps['tail'].nrows, rowmap=maps['tail'])
        else:
            K.gemm_rms(OT_GEMM_NT, dy2, d, d, mt['rows'][1], m.p(f'blk.{l}.w2'), f * d, d, f, mt['tile_group'], nt, du,
                       f, mt['rows'][1], epi=OT_EPI_GELU_BWD, aux=s.u, ldaux=f, m_rows=maps['tail'].nrows, device=dev,
                       bimg=m.bimg(f'blk.{l}.w2', 'dgrad'), **rep_du, **pa2)
        pa1 = a_row_bounds(form.pw1, du, f, B * Kq, f, rm_du) if not ffn_bwd else {}
        a1, ax_1 = (s.x1n, OT_AX_BF16) if form.a1n else (s.x1, OT_AX_RMSNORM)   # both operands bf16: copy-staged
        with m.side(a1, du, s.rstd2, *keep):
            K.wgrad(a1, d, mt['rows'][1], du, f, mt['rows'][1], d, f, mt, nct, G, m.g(f'blk.{l}.w1'),
                    d * f, m.g(f'blk.{l}.b1'), f, rstd=s.rstd2, gamma=m.p(f'blk.{l}.norm2'),
                    a_xform=ax_1 | (OT_WG_D_BF16 if du_bf else 0),
                    accumulate=acc, device=dev, m_rows=maps['tail'].nrows, rowmap=maps['tail'], d_bound=b_du)
        # FFN1 dgrad -> norm2 backward + residual; emit mask(dx1) for the attention branch
        # (with ffn_bwd, dx1 / dyo and their reports came from the fused launch above)
        if not form.dx1_ep:
            dxn2 = torch.empty(B * Kq, d, device=dev)
            K.gemm_rms(OT_GEMM_NT, du, f, f, mt['rows'][1], m.p(f'blk.{l}.w1'), d * f, f, d, mt['tile_group'], nt,
                       dxn2, d, mt['rows'][1], epi=0, m_rows=maps['tail'].nrows, device=dev,
                       bimg=m.bimg(f'blk.{l}.w1', 'dgrad'), **pa1)
            K.rmsnorm_bwd(dxn2, d, s.x1, d, m.p(f'blk.{l}.norm2'), s.rstd2, dx1, d, B * Kq, d, dres=dx2, lddres=d,
                          dx_masked=dyo if rate > 0 else None, lddxm=d, seed=seed, site=2 * l, drop=rate,
                          tail=tail, dgamma=m.g(f'blk.{l}.norm2'), accumulate=acc, device=dev)
        elif not ffn_bwd:
            K.gemm_rms(OT_GEMM_NT, du, f, f, mt['rows'][1], m.p(f'blk.{l}.w1'), d * f, f, d, mt['tile_group'], nt,
                       dx1, d, mt['rows'][1], epi=OT_EPI_RMSNORM_BWD | (OT_EPI_DROPOUT if rate > 0 else 0),
                       a_xform=OT_AX_BF16 if du_bf else 0,
                       seed=seed, site=2 * l, drop=rate, tail=tail, m_rows=maps['tail'].nrows, nx=s.x1, ldnx=d,
                       ngamma=m.p(f'blk.{l}.norm2'), nrstd=s.rstd2, dres=dx2, lddres=d,
                       dx_masked=dyo if rate > 0 else None, lddxm=d, dgamma=m.g(f'blk.{l}.norm2'),
                       accumulate_dgamma=acc, device=dev, bimg=m.bimg(f'blk.{l}.w1', 'dgrad'),
                       rowdot=rowdot, rowdot_n=f // TILE if rowdot is not None else 0, amax_out=b_dyo,
                       rowabs_out=rm_dyo, rowabs_n=rm_dyo.shape[1] if rm_dyo is not None else 0, **pa1)
        # Wo
        with m.side(s.o, dyo, *keep):
            _wgrad_single(m, s.o, dyo, d, d, mt, m.g(f'blk.{l}.wo'), acc, dev, maps['tail'].nrows, maps['tail'],
                          a_bound=b_o, d_bound=b_dyo)
        do = torch.empty(B * Kq, d, device=dev)
        K.gemm_rms(OT_GEMM_NT, dyo, d, d, mt['rows'][1], m.p(f'blk.{l}.wo'), 0, d, d, mt['tile_group'], nt, do, d,
                   mt['rows'][1], epi=0, m_rows=maps['tail'].nrows, device=dev, bimg=m.bimg(f'blk.{l}.wo', 'dgrad'),
                   **a_row_bounds(form.pwo, dyo, d, B * Kq, d, rm_dyo))
        if fwd.fold is not None:     # the forward took the folded one-query attention
            dx = _fold_backward(m, l, s, do, dx1, B, I, maps['fold'], acc, dev, form.pqkv)
            m.side_block_done()
            if m.grad_ready is not None:
                m.grad_ready(l)
            return None, dx, None, None, None, None, None, None, None, None, None, None
        # attention
        qp = _attn_qpos(cfg, pos)
        dq_bf, pqkv = form.dq_bf, form.pqkv
        dqkv = torch.empty(B * I, 3 * d, device=dev, dtype=torch.int16 if dq_bf else torch.float32)
        if Kq < I:
            dqkv[:, :d].zero_()
        b_dq = out('dqkv') if form.dq_rep else None
        # the QKV dgrad on the fp16 pair: dQKV's row maxima [row][q / k / v][head] from the attention backward (the
        # dQ part of rows without a query stays 0), else the row-absmax pass
        rm_dq = torch.zeros(B * I, 3 * H, device=dev) if pqkv and form.dq_rep else None
        if kvalid is not None:
            K.attn_bwd_masked(s.qkv, 3 * d, s.o, do, s.lse, B, H, I, Kq, hd, dqkv, _layer_valid(kvalid, I), qpos=qp)
        else:
            K.attn_bwd(s.qkv, 3 * d, s.o, do, s.lse, B, H, I, Kq, hd, dqkv, qpos=qp, dq_part_bf16=True, amax=b_dq,
                       rowmax=rm_dq)
        pa_q = a_row_bounds(pqkv, dqkv, 3 * d, B * I, 3 * d, rm_dq)
        aq, ax_q = (s.xn1, OT_AX_BF16) if form.an1 else (s.x, OT_AX_RMSNORM)
        with m.side(aq, dqkv, s.rstd1, *keep):
            K.wgrad(aq, d, ma['rows'][0], dqkv, 3 * d, ma['rows'][0], d, 3 * d, ma, nca, G,
                    m.g(f'blk.{l}.wqkv'), 3 * d * d, None, 0, a_xform=ax_q | (OT_WG_D_BF16 if dq_bf else 0),
                    rstd=s.rstd1, gamma=m.p(f'blk.{l}.norm1'), accumulate=acc, device=dev, m_rows=maps['all'].nrows,
                    rowmap=maps['all'], d_bound=b_dq)
        ax_dq = OT_AX_BF16 if dq_bf else 0
        dx = torch.empty(B * I, d, device=dev)
        if form.qkv_ep:         # QKV dgrad -> norm1 backward + residual (dx1 on the kept tail rows)
            # the block below masks dx inside its fused FFN backward: this launch reports dx's row maxima and bound
            rep_dx = {}
            if form.rep_dx:
                rm_dx = torch.empty(B * I, 1, device=dev)
                rep_dx = dict(amax_out=out('dx'), rowabs_out=rm_dx, rowabs_n=1)
            K.gemm_rms(OT_GEMM_NT, dqkv, 3 * d, 3 * d, ma['rows'][0], m.p(f'blk.{l}.wqkv'), 3 * d * d, 3 * d, d,
                       ma['tile_group'], na, dx, d, ma['rows'][0], epi=OT_EPI_RMSNORM_BWD, a_xform=ax_dq,
                       m_rows=maps['all'].nrows, nx=s.x, ldnx=d, ngamma=m.p(f'blk.{l}.norm1'), nrstd=s.rstd1,
                       dres=dx1, lddres=d, dres_tail=(Kq, I, inv) if Kq < I else (0, 0),
                       dgamma=m.g(f'blk.{l}.norm1'), accumulate_dgamma=acc, device=dev,
                       bimg=m.bimg(f'blk.{l}.wqkv', 'dgrad'), **pa_q, **rep_dx)
            if rep_dx:
                bounds.put_dx(l, dx, rm_dx)
        else:
            dxn1 = torch.empty(B * I, d, device=dev)
            K.gemm_rms(OT_GEMM_NT, dqkv, 3 * d, 3 * d, ma['rows'][0], m.p(f'blk.{l}.wqkv'), 3 * d * d, 3 * d, d,
                       ma['tile_group'], na, dxn1, d, ma['rows'][0], epi=0, m_rows=maps['all'].nrows, a_xform=ax_dq,
                       bimg=m.bimg(f'blk.{l}.wqkv', 'dgrad'), device=dev, **pa_q)
            K.rmsnorm_bwd(dxn1, d, s.x, d, m.p(f'blk.{l}.norm1'), s.rstd1, dx, d, B * I, d, dres=dx1, lddres=d,
                          dres_tail=(Kq, I, inv) if Kq < I else (0, 0), dgamma=m.g(f'blk.{l}.norm1'), accumulate=acc,
                          device=dev)
        m.side_block_done()
        if m.grad_ready is not None:
            m.grad_ready(l)                     # this block's banks are final: the DP exchange may start
        return None, dx, None, None, None, None, None, None, None, None, None, None


def _fold_backward(m, l, s: BlockSaved, do, dx1, B, I, fmap, acc, dev, pqkv: bool):
    """Backward of the folded one-query attention and of the QKV projection around it (``fold_gate``): the fold
    kernel streams x once and writes dx of every row (norm1's backward applied; + dx1 on the query row); dQKV exists
    only for the ``fold`` map's rows (the dedicated keys and the query), compact, and the QKV dgrad adds their part
    onto the dx rows in place; the Wqkv weight gradient runs over those rows, and group 0's dWk / dWv — the keys that
    were never projected — come from z / y (ot_attn_fold_dw).  No PairBounds slots: these few-thousand-row weight
    gradients run the exact split.  ``pqkv``: Wqkv's dgrad image is in the pair form.  Returns dx [B*I, d]."""
    cfg = m.config
    d, H, G = cfg.hidden_dim, cfg.num_heads, cfg.num_groups
    hd = d // H
    x, rstd1, qkv, yf = s.x, s.rstd1, s.qkv, s.yf
    ded = m.fold_ded(I)
    mf = fmap.to(dev)
    nf = K.attn_fold_rows(I, *ded)
    g1, w = m.p(f'blk.{l}.norm1'), m.p(f'blk.{l}.wqkv')
    dqkv = torch.empty(B * nf, 3 * d, device=dev)
    dx = torch.empty(B * I, d, device=dev)
    zf = torch.empty(B * H, d, device=dev)
    dgp = torch.empty(B, d, device=dev)
    K.attn_fold_bwd(x, d, rstd1, g1, w, 3 * d, m.pT(f'blk.{l}.wqkv'), d, qkv, 3 * d, B, H, I, hd, ded, s.o, do, s.lse,
                    yf, dx1, dx, d, dqkv, 3 * d, zf, dgp)
    pa_q = a_row_bounds(pqkv, dqkv, 3 * d, B * nf, 3 * d)
    K.gemm_rms(OT_GEMM_NT, dqkv, 3 * d, 3 * d, mf['rows'][1], w, 3 * d * d, 3 * d, d, mf['tile_group'], fmap.ntiles,
               dx, d, mf['rows'][0], epi=OT_EPI_RMSNORM_BWD, m_rows=fmap.nrows, nx=x, ldnx=d, ngamma=g1, nrstd=rstd1,
               dres=dx, lddres=d, dgamma=m.g(f'blk.{l}.norm1'), accumulate_dgamma=acc, device=dev,
               bimg=m.bimg(f'blk.{l}.wqkv', 'dgrad'), **pa_q)
    K.attn_fold_dgamma(dgp, B, d, m.g(f'blk.{l}.norm1'), accumulate=True)
    with m.side(x, dqkv, rstd1, zf, yf, qkv, do):
        K.wgrad(x, d, mf['rows'][0], dqkv, 3 * d, mf['rows'][1], d, 3 * d, mf, fmap.chunks.shape[0], G,
                m.g(f'blk.{l}.wqkv'), 3 * d * d, None, 0, a_xform=OT_AX_RMSNORM, rstd=rstd1, gamma=g1, accumulate=acc,
                device=dev, m_rows=fmap.nrows, rowmap=fmap)
        K.attn_fold_dw(zf, yf, qkv, 3 * d, do, g1, B, H, I, hd, m.g(f'blk.{l}.wqkv'), 3 * d, accumulate=True)
    return dx


def _wgrad_single(m, A, D, K_, N, mt, dW, acc, dev, mrows=0, rowmap=None, a_bound=None, d_bound=None):
    """Wo gradient: one weight shared by every group -> wgrad with every chunk mapped to group 0
    (chunked by layout.wgrad_slots for its single output tile when the row map is given)."""
    if rowmap is not None and rowmap.group_rows:
        ch, _, _ = rowmap.chunks_for(((K_ + 127) // 128) * ((N + 127) // 128), dev)
        mp = m.single_group_chunks({'chunks': ch})
    else:
        mp = m.single_group_chunks(mt)
    K.wgrad(A, K_, mt['rows'][1], D, N, mt['rows'][1], K_, N, mp, mp['chunks'].shape[0], 1, dW, 0, None, 0,
            accumulate=acc, device=dev, m_rows=mrows, a_bound=a_bound, d_bound=d_bound)
