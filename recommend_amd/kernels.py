"""Thin torch-tensor wrappers over the C ABI (``_lib``).  No arithmetic happens here: every
function forwards device pointers, sizes and the current HIP stream to libonetrans_hip.so.

Pointer arguments accept a tensor, ``(tensor, element_offset)`` or None."""

from __future__ import annotations

import contextlib
import ctypes
import functools
import os
import threading
from typing import Optional, Tuple, Union

import torch

from . import _lib
from ._lib import call, size

Ptrish = Union[None, torch.Tensor, Tuple[torch.Tensor, int]]


class Probe:
    """Times kernel launches with HIP events recorded on the launch stream (bench.py uses it over
    the timed region) and accumulates the algorithmic FLOPs of each launch (valid rows only)."""

    def __init__(self):
        self.recs = []

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, family: str, flops: float, ev0, label: str = '', nbytes: float = 0.0, terms: int = 0) -> None:
        """``terms``: 16-bit MFMA products per f32 product the launch issues (6 split-bf16, 3 fp16 pair, 1 bf16; 0 =
        the family's default peak) — its launch is floored against that arithmetic's ceiling."""
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        self.recs.append((family, flops, ev0, ev1, label, nbytes, terms))

    def by_label(self, steps: int):
        """Per-launch-shape breakdown: {label: (launches/step, avg us, TF/s)} (tools/gemm_shapes.py)."""
        torch.cuda.synchronize()
        agg = {}
        for rec in self.recs:
            f, fl, a, b, lab = rec[:5]
            d = agg.setdefault(f'{f} {lab}', [0, 0.0, 0.0])
            d[0] += 1
            d[1] += a.elapsed_time(b)
            d[2] += fl
        return {k: (n / steps, 1e3 * ms / n, fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0)
                for k, (n, ms, fl) in agg.items()}

    def report(self, steps: int, mfma_peak_tflops: float = 0.0, hbm_peak_gbs: float = 0.0, terms_peak=None):
        """Per family: time, launches, algorithmic FLOPs and bytes per launch; with the peaks given, also
        the family's roofline floor sum_i max(flops_i / mfma peak_i, bytes_i / HBM peak) over its launches
        (each launch bound by whichever roof it meets first) and the MFMA / HBM parts of it.  ``terms_peak(t)``: the
        MFMA ceiling (f32 TF/s) of a launch issuing t products per f32 product (its recorded ``terms``); the family's
        ``mfma_peak_eff`` = its flops over the sum of flops_i / peak_i (the ceiling of the arithmetic it issued)."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        fam = {}
        for rec in self.recs:
            f, fl, a, b, _, nb = rec[:6]
            terms = rec[6] if len(rec) > 6 else 0
            d = fam.setdefault(f, {'ms': 0.0, 'flops': 0.0, 'bytes': 0.0, 'n': 0, 'floor': 0.0, 'fl_mfma': 0.0,
                                   'fl_hbm': 0.0, 'mfma_ms': 0.0, 'pair': 0})
            d['ms'] += a.elapsed_time(b)
            d['flops'] += fl
            d['bytes'] += nb
            d['n'] += 1
            d['pair'] += terms == 3
            if mfma_peak_tflops > 0 and hbm_peak_gbs > 0:
                pk = terms_peak(terms) if (terms_peak is not None and terms) else mfma_peak_tflops
                tm, th = fl / (pk * 1e9), nb / (hbm_peak_gbs * 1e6)     # ms
                d['mfma_ms'] += tm
                d['floor'] += max(tm, th)
                d['fl_mfma' if tm >= th else 'fl_hbm'] += max(tm, th)
        out = {}
        for f, d in fam.items():
            out[f] = {'ms_per_step': d['ms'] / steps, 'avg_us': 1e3 * d['ms'] / d['n'],
                      'launches_per_step': d['n'] / steps, 'gflop_per_launch': d['flops'] / d['n'] / 1e9,
                      'gbyte_per_launch': d['bytes'] / d['n'] / 1e9,
                      'tflops': d['flops'] / (d['ms'] * 1e-3) / 1e12 if d['ms'] > 0 else 0.0,
                      'gbs': d['bytes'] / (d['ms'] * 1e-3) / 1e9 if d['ms'] > 0 else 0.0,
                      'floor_ms_per_step': d['floor'] / steps, 'floor_mfma_ms_per_step': d['fl_mfma'] / steps,
                      'floor_hbm_ms_per_step': d['fl_hbm'] / steps,
                      'mfma_peak_eff': d['flops'] / (d['mfma_ms'] * 1e9) if d['mfma_ms'] > 0 else 0.0,
                      'pair_launches_per_step': d['pair'] / steps}
        return {'families': out}


_probe = None


def _terms(bimg, a_xform: int, a_rowmax, N: int) -> int:
    """MFMA products per f32 product a forward / dgrad launch issues (the probe's ceiling): bf16 mode 1, f32 mode 0
    (native), split mode 3 on the plane GEMM's fp16 pair (RMSNorm prologue, or A row maxima given), else 6."""
    mm = matmul_mode()
    if mm != 'split':
        return 1 if mm == 'bf16' else 0
    pair = bimg is not None and N % 128 == 0 and (
        a_xform == _lib.OT_AX_RMSNORM or (a_rowmax is not None and a_xform in (_lib.OT_AX_NONE, _lib.OT_AX_GELU)))
    return 3 if pair else 6


def gemm_bytes(M: int, K: int, N: int, a_xform: int, epi: int) -> float:
    """Algorithmic HBM bytes of one forward / dgrad GEMM launch over M valid rows: A read once (+ its
    rstd for the RMSNorm prologue), C written once, each [M, N] epilogue operand read once.  Weights
    (at most a few MB of L2-resident images) are left out."""
    mn = (1 + bool(epi & _lib.OT_EPI_RESIDUAL) + bool(epi & _lib.OT_EPI_GELU_BWD)
          + bool(epi & _lib.OT_EPI_ACCUMULATE))
    a_bytes = 2.0 if a_xform in (_lib.OT_AX_BF16, _lib.OT_AX_BF16_RMSNORM) else 4.0   # bf16 A operands
    c_less = 2.0 * M * N if epi & _lib.OT_EPI_C_BF16 else 0.0       # OT_EPI_C_BF16: C written in bf16
    return a_bytes * M * K + 4.0 * M * (a_xform == _lib.OT_AX_RMSNORM) + 4.0 * M * N * mn - c_less


def set_probe(p) -> None:
    global _probe
    _probe = p


# Matmul arithmetic is an argument of every GEMM / weight-gradient / plane-image / attention call (the C ABI
# holds no precision state).  The wrappers below pass the innermost ``precision(...)`` scope of the calling
# thread (a model enters its own: OneTransModel.matmul, from cfg.compute_dtype), else the process default
# (``set_matmul_mode``; initially ONETRANS_MATMUL, 'split').
_default_mode = os.environ.get('ONETRANS_MATMUL', 'split')
if _default_mode not in _lib.MATMUL_MODES:
    raise _lib.OneTransHipError(f'ONETRANS_MATMUL={_default_mode!r}: expected one of {sorted(_lib.MATMUL_MODES)}')
_scope = threading.local()


def set_matmul_mode(mode: str) -> str:
    """Process-default GEMM / attention arithmetic for calls outside a ``precision`` scope: 'split' (exact
    3-way bf16 split on bf16 MFMA, f32-accurate), 'f32' (native f32 MFMA) or 'bf16'.  Returns the previous.
    A model reads the default once, at construction (OneTransModel.matmul): models that exist keep their mode."""
    global _default_mode
    if mode not in _lib.MATMUL_MODES:
        raise ValueError(f'matmul mode {mode!r}: expected one of {sorted(_lib.MATMUL_MODES)}')
    old, _default_mode = _default_mode, mode
    return old


def matmul_mode() -> str:
    """The arithmetic the next call on this thread uses."""
    st = getattr(_scope, 'stack', None)
    return st[-1] if st else _default_mode


@contextlib.contextmanager
def precision(mode: str):
    """Calls on this thread inside the block use ``mode``."""
    if mode not in _lib.MATMUL_MODES:
        raise ValueError(f'matmul mode {mode!r}: expected one of {sorted(_lib.MATMUL_MODES)}')
    st = getattr(_scope, 'stack', None)
    if st is None:
        st = _scope.stack = []
    st.append(mode)
    try:
        yield
    finally:
        st.pop()


def _prec() -> int:
    return _lib.MATMUL_MODES[matmul_mode()]


def precision_owner(obj):
    """The model whose arithmetic a method of ``obj`` runs in: ``obj`` itself when it carries a matmul mode
    (``OneTransModel``), else the object's ``precision_model`` (serving engines, trainers: a property naming
    the model they drive)."""
    if isinstance(getattr(obj, 'matmul', None), str):
        return obj
    owner = getattr(type(obj), 'precision_model', None)
    if owner is None:
        raise TypeError(f'{type(obj).__name__}: in_model_precision needs a .matmul mode or a precision_model property')
    owner = owner.__get__(obj)
    if not isinstance(getattr(owner, 'matmul', None), str):
        raise TypeError(f'{type(obj).__name__}.precision_model has no matmul mode')
    return owner


def in_model_precision(fn):
    """Run a method of a model (``.matmul``) or of an object driving one (``precision_model``) inside that
    model's ``precision`` scope: every GEMM / attention call it makes carries the model's arithmetic."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kw):
        with precision(precision_owner(self).matmul):
            return fn(self, *args, **kw)
    return wrapped


def ptr(x: Ptrish):
    if x is None:
        return None
    if isinstance(x, tuple):
        t, off = x
        return t.data_ptr() + off * t.element_size()
    return x.data_ptr()


def _sel(tail):
    """Kept-token map of a (K, I[, map]) tail spec: the third element (a device int32 tensor from
    ``pyramid_select``: positions for ``tail``, inverse rows for ``dres_tail``) or None (the tail rule)."""
    return ptr(tail[2]) if len(tail) > 2 and tail[2] is not None else None


def pyramid_select(B: int, I: int, K: int, pos: torch.Tensor, inv: Optional[torch.Tensor] = None,
                   score: Optional[torch.Tensor] = None, sign: float = 1.0, nforce: int = 0,
                   map_rows: Optional[torch.Tensor] = None, map_per_sample: int = 0) -> None:
    """ot_pyramid_select: per-sample top-K positions (ascending) by score*sign, the last ``nforce`` kept;
    no score = the tail (model.py:287-302, 371)."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_pyramid_select', ptr(score), float(sign), B, I, K, nforce, ptr(pos), ptr(inv), ptr(map_rows),
         map_per_sample, stream())
    if ev is not None:
        _probe.end('pyramid', 0.0, ev)


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def gemm(mode: int, A: Ptrish, lda: int, K: int, in_rows: Ptrish, W: Ptrish, w_gstride: int, ldw: int, N: int,
         tile_group: Ptrish, ntiles: int, C: Ptrish, ldc: int, out_rows: Ptrish, *, a_xform: int = 0,
         rstd: Ptrish = None, gamma: Ptrish = None, bias: Ptrish = None, bias_gstride: int = 0, epi: int = 0,
         res: Ptrish = None, ldres: int = 0, res_tok: int = 0, aux: Ptrish = None, ldaux: int = 0,
         seed: int = 0, site: int = 0, drop: float = 0.0, tail: Tuple[int, int] = (1, 1),
         m_rows: int = 0, bimg=None) -> None:
    """ot_mixed_gemm; ``bimg`` = (image, tiles per group, first tile) of B's pre-split image
    (ot_mixed_gemm_img: the plane GEMM in split mode)."""
    ev = _probe.begin() if _probe is not None else None
    args = (mode, ptr(A), lda, K, ptr(in_rows), a_xform, ptr(rstd), ptr(gamma), ptr(W), w_gstride,
            ldw, N, ptr(tile_group), ntiles, ptr(bias), bias_gstride, ptr(C), ldc, ptr(out_rows), epi, ptr(res),
            ldres, res_tok, ptr(aux), ldaux, seed & 0xFFFFFFFF, site, float(drop), tail[0], tail[1], _sel(tail))
    if bimg is not None:
        call('ot_mixed_gemm_img', *args, ptr(bimg[0]), bimg[1], bimg[2], _prec(), stream())
    else:
        call('ot_mixed_gemm', *args, _prec(), stream())
    if ev is not None:
        M = m_rows or ntiles * 128
        _probe.end('mixed_gemm', 2.0 * M * K * N, ev, f'gemm mode{mode} ax{a_xform} epi{epi} M{M} K{K} N{N}',
                   gemm_bytes(M, K, N, a_xform, epi), _terms(bimg, a_xform, None, N))


def gemm_rms(mode: int, A: Ptrish, lda: int, K: int, in_rows: Ptrish, W: Ptrish, w_gstride: int, ldw: int,
             N: int, tile_group: Ptrish, ntiles: int, C: Ptrish, ldc: int, out_rows: Ptrish, *, epi: int,
             a_xform: int = 0, rstd: Ptrish = None, gamma: Ptrish = None, bias: Ptrish = None,
             bias_gstride: int = 0, res: Ptrish = None, ldres: int = 0, res_tok: int = 0, seed: int = 0,
             site: int = 0, drop: float = 0.0, tail: Tuple[int, int] = (1, 1), m_rows: int = 0,
             rstd_out: Ptrish = None, eps: float = 1e-6, nx: Ptrish = None, ldnx: int = 0,
             ngamma: Ptrish = None, nrstd: Ptrish = None, dres: Ptrish = None, lddres: int = 0,
             dres_tail: Tuple[int, int] = (0, 0), dx_masked: Ptrish = None, lddxm: int = 0,
             dgamma: Ptrish = None, accumulate_dgamma: bool = False, device=None, bimg=None,
             aux: Ptrish = None, ldaux: int = 0, rowdot: Ptrish = None, rowdot_n: int = 0,
             gelu_out: Ptrish = None, ldgelu: int = 0, xn_out: Ptrish = None, ldxn: int = 0,
             c16_out: Ptrish = None, ldc16: int = 0, rowmax_out: Ptrish = None, rowmax_n: int = 0,
             a_rowmax: Ptrish = None, a_rowmax_n: int = 0, amax_out: Ptrish = None, rowabs_out: Ptrish = None,
             rowabs_n: int = 0) -> None:
    """ot_mixed_gemm_rms: the GEMM with a row-norm epilogue (OT_EPI_ROW_RSTD: emit the next RMSNorm's
    rstd; OT_EPI_RMSNORM_BWD: apply the RMSNorm backward to the product, + dres, dgamma, taking
    <gamma dy, x> from ``rowdot`` when N > 128; OT_EPI_GELU_BWD | OT_EPI_ROWDOT: also write each 128-column
    tile's sum of dU (aux - bias) into rowdot[row][tile]); ``gelu_out`` (bf16 bits, [rows][ldgelu]) also
    receives gelu(aux) (with OT_EPI_GELU_BWD) or gelu(C) (epi == OT_EPI_BIAS: the FFN1 forward) rounded to
    bf16 — the OT_AX_BF16 operand of the FFN2 GEMM and the W2 weight gradient.  ``xn_out`` (bf16 bits,
    [in rows][ldxn]; RMSNorm prologue, plane GEMM) receives bf16((A * gamma) * rstd): the normalised A
    operand of the bf16 weight gradient.  ``rowmax_out`` ([out rows][N / 128], split-mode plane GEMM) receives
    each column tile's largest C after the bias (the FFN1 forward's U); ``a_rowmax`` hands such maxima of A to a
    GELU-prologue plane GEMM, which then multiplies on the scaled fp16 pair (its image in the pair form)."""
    need_ws = dgamma is not None or (rstd_out is not None and N > 128)     # dgamma / row-sum partials
    ws = workspace(size('ot_mixed_gemm_rms_workspace_size', ntiles, N) if need_ws else 16,
                   device if device is not None else (C[0] if isinstance(C, tuple) else C).device)
    e = _lib.RmsEpilogue(ctypes.sizeof(_lib.RmsEpilogue), ptr(rstd_out), float(eps), ptr(nx), ldnx, ptr(ngamma), ptr(nrstd), ptr(dres), lddres,
                         dres_tail[0], dres_tail[1], _sel(dres_tail), ptr(dx_masked), lddxm, ptr(dgamma),
                         int(accumulate_dgamma), ptr(ws), ws.numel(), ptr(rowdot), int(rowdot_n),
                         ptr(gelu_out), int(ldgelu), ptr(xn_out), int(ldxn), ptr(c16_out), int(ldc16),
                         ptr(rowmax_out), int(rowmax_n), ptr(a_rowmax), int(a_rowmax_n), ptr(amax_out),
                         ptr(rowabs_out), int(rowabs_n))
    ev = _probe.begin() if _probe is not None else None
    args = (mode, ptr(A), lda, K, ptr(in_rows), a_xform, ptr(rstd), ptr(gamma), ptr(W),
            w_gstride, ldw, N, ptr(tile_group), ntiles, ptr(bias), bias_gstride, ptr(C), ldc, ptr(out_rows), epi,
            ptr(res), ldres, res_tok, ptr(aux), ldaux, seed & 0xFFFFFFFF, site, float(drop), tail[0], tail[1],
            _sel(tail), ctypes.byref(e))
    if bimg is not None:
        call('ot_mixed_gemm_rms_img', *args, ptr(bimg[0]), bimg[1], bimg[2], _prec(), stream())
    else:
        call('ot_mixed_gemm_rms', *args, _prec(), stream())
    if ev is not None:
        M = m_rows or ntiles * 128
        extra = (nx is not None) + (dres is not None) + (dx_masked is not None)   # norm-backward operands
        _probe.end('mixed_gemm', 2.0 * M * K * N, ev, f'gemm_rms mode{mode} ax{a_xform} epi{epi} M{M} K{K} N{N}',
                   gemm_bytes(M, K, N, a_xform, epi) + 4.0 * M * N * extra + 2.0 * M * N * (gelu_out is not None)
                   + 2.0 * M * K * (xn_out is not None)
                   + 4.0 * M * ((rstd_out is not None) + (nrstd is not None)), _terms(bimg, a_xform, a_rowmax, N))


def wgrad(A: Ptrish, lda: int, a_rows: Ptrish, D: Ptrish, ldd: int, d_rows: Ptrish, K: int, N: int, rmap_dev,
          nchunks: int, ngroups: int, dW: Ptrish, dw_gstride: int, db: Ptrish = None, db_gstride: int = 0, *,
          a_xform: int = 0, rstd: Ptrish = None, gamma: Ptrish = None, accumulate: bool = False,
          device=None, m_rows: int = 0, rowmap=None, a_bound: Ptrish = None, d_bound: Ptrish = None,
          keep: Ptrish = None, ldkeep: int = 0, d_scale: float = 1.0) -> None:
    """rmap_dev: dict with 'chunks'/'gchunk' device tensors; when ``rowmap`` (a layout.RowMap) is given
    its chunking is re-balanced for this call's output tile count (layout.wgrad_slots).  ``d_bound`` / ``a_bound``
    (one float each on the device, from the operands' producers): the split mode runs the fp16-pair kernel
    (ot_mixed_gemm_wgrad_ex; the RMSNorm prologue's A needs no bound).  ``keep`` (with ``a_xform`` OT_AX_GELU |
    OT_WG_D_KEEPBITS; ot_mixed_gemm_wgrad_keep): D is the gradient before a dropout mask, masked and scaled by
    ``d_scale`` at staging time from the rows' keep bits; ``d_bound`` then bounds the unmasked |D|."""
    if rowmap is not None and rowmap.group_rows:
        tiles = ((K + 127) // 128) * ((N + 127) // 128)
        ch, gc, nchunks = rowmap.chunks_for(tiles, device)
        rmap_dev = {'chunks': ch, 'gchunk': gc}
    nbytes = size('ot_wgrad_workspace_size', nchunks, K, N)
    ws = workspace(nbytes, device)
    ev = _probe.begin() if _probe is not None else None
    if keep is not None:
        assert rstd is None and gamma is None
        call('ot_mixed_gemm_wgrad_keep', ptr(A), lda, ptr(a_rows), a_xform, ptr(D), ldd, ptr(d_rows), K, N,
             ptr(rmap_dev['chunks']), nchunks, ptr(rmap_dev['gchunk']), ngroups, ptr(dW), dw_gstride, ptr(db),
             db_gstride, int(accumulate), ptr(ws), ws.numel(), ptr(a_bound), ptr(d_bound), ptr(keep), ldkeep,
             float(d_scale), _prec(), stream())
        a_xform &= ~_lib.OT_WG_D_KEEPBITS
    else:
        call('ot_mixed_gemm_wgrad_ex', ptr(A), lda, ptr(a_rows), a_xform, ptr(rstd), ptr(gamma), ptr(D), ldd,
             ptr(d_rows), K, N, ptr(rmap_dev['chunks']), nchunks, ptr(rmap_dev['gchunk']), ngroups, ptr(dW),
             dw_gstride, ptr(db), db_gstride, int(accumulate), ptr(ws), ws.numel(), ptr(a_bound), ptr(d_bound),
             _prec(), stream())
    if ev is not None:
        ax = a_xform & ~_lib.OT_WG_D_BF16
        wterms = {'bf16': 1, 'f32': 0}.get(matmul_mode(), 3 if (
            d_bound is not None and not (a_xform & _lib.OT_WG_D_BF16)
            and (ax == _lib.OT_AX_RMSNORM or (a_bound is not None and ax in (_lib.OT_AX_NONE, _lib.OT_AX_GELU))))
            else 6)
        _probe.end('mixed_gemm', 2.0 * m_rows * K * N, ev, f'wgrad ax{a_xform} M{m_rows} K{K} N{N} ch{nchunks}',
                   (2.0 if (a_xform & ~_lib.OT_WG_D_BF16) == _lib.OT_AX_BF16 else 4.0) * m_rows * K
                   + (2.0 if a_xform & _lib.OT_WG_D_BF16 else 4.0) * m_rows * N
                   + 4.0 * m_rows * ((a_xform & ~_lib.OT_WG_D_BF16) == _lib.OT_AX_RMSNORM) + 4.0 * ngroups * K * N,
                   wterms)


def transpose_banks(src, dst, banks_dev, nbanks, total_tiles) -> None:
    call('ot_transpose_banks', ptr(src), ptr(dst), ptr(banks_dev), nbanks, total_tiles, stream())


def split_image_elems(G: int, N: int, K: int) -> int:
    return int(_lib.load().ot_split_image_elems(G, N, K))


def plane_wide(on: int = -1) -> int:
    """ot_plane_wide: the bf16-mode plane GEMM's tile process-wide — 0: 128 x 128, 1: auto (default), 2 / 3 / 4:
    128 x 256 / 128 x 512 / 256 x 256 where the shape allows — or query (-1); returns the previous setting (a tuning
    / test knob: every tile gives bit-identical outputs)."""
    return _lib.size('ot_plane_wide', int(on))


def wgrad_wide(on: int = -1) -> int:
    """ot_wgrad_wide: the bf16 weight gradient's tile — 0: 128 x 128, 1: auto (default), 2: 128 x 256, 3: 256 x 256
    where K and N allow — or query (-1); returns the previous setting (bit-identical slabs either way)."""
    return _lib.size('ot_wgrad_wide', int(on))


def plane_rowmeta(on: int = -1) -> int:
    """ot_plane_rowmeta: the pair plane GEMM's epilogue row metadata — 1: parked in LDS once per tile (default), 0:
    read from the row maps per row batch — or query (-1); returns the previous setting (bit-identical outputs)."""
    return _lib.size('ot_plane_rowmeta', int(on))


def plane_panel(on: int = -1) -> int:
    """ot_plane_panel: the panel form of the pair plane GEMM (one workgroup per row tile walks its column tiles) — 0:
    off (default), 1: auto, w in 2 .. 64: w column tiles per workgroup, 100 + w: the four-workgroups-per-CU variant,
    200 + w: A's fragments held across the column tiles (K = 128) — or query (-1); returns the previous setting
    (bit-identical outputs)."""
    return _lib.size('ot_plane_panel', int(on))


def plane_panel_launches() -> int:
    """ot_plane_panel_launches: GEMM launches that took the panel form since the library was loaded."""
    return _lib.size('ot_plane_panel_launches')


def ffn_fused(on: int = -1) -> int:
    """ot_ffn_fused: whether the block forward takes the fused FFN kernel where its form applies (split mode, hidden
    width 128, pair-form W1 / W2 forward images, ffn width a multiple of 128 up to ``FFN_FUSED_MAX_F``) — 1 (default)
    or 0: the FFN1 and FFN2 launches — or query (-1); returns the previous setting."""
    return _lib.size('ot_ffn_fused', int(on))


FFN_FUSED_MAX_F = 1024


def ffn_fused_fwd(x1: Ptrish, ldx1: int, rows: Ptrish, tile_group: Ptrish, ntiles: int, rstd: Ptrish, w1_image,
                  w1_groups: int, w2_image, w2_groups: int, b1: Ptrish, b1_gstride: int, b2: Ptrish, b2_gstride: int,
                  f: int, x2: Ptrish, ldx2: int, *, u_out: Ptrish = None, ldu: int = 0, u_amax: Ptrish = None,
                  rstd_out: Ptrish = None, eps: float = 1e-6, seed: int = 0, site: int = 0, drop: float = 0.0,
                  tail: Tuple[int, int] = (1, 1), m_rows: int = 0) -> None:
    """ot_ffn_fused_fwd: x2 = x1 + drop(gelu(rstd * (x1 @ gamma W1[g]) + b1[g]) @ W2[g] + b2[g]) for rows of 128
    floats in one launch (split mode; ``w1_image`` / ``w2_image``: the pair-form forward images as ``(tensor,
    element offset)``); ``u_out`` also receives the pre-activation (bit for bit the FFN1 launch's), ``u_amax`` its
    max |u|, ``rstd_out`` the rstd of the x2 rows."""
    a = _lib.FfnFusedArgs(ctypes.sizeof(_lib.FfnFusedArgs), ptr(x1), ldx1, ptr(rows), ptr(tile_group), ntiles,
                          ptr(rstd), ptr(w1_image), int(w1_groups), ptr(w2_image), int(w2_groups), ptr(b1),
                          b1_gstride, ptr(b2), b2_gstride, f, ptr(u_out), ldu, ptr(u_amax), ptr(x2), ldx2,
                          ptr(rstd_out), float(eps), seed & 0xFFFFFFFF, site, float(drop), tail[0], tail[1],
                          _sel(tail))
    ev = _probe.begin() if _probe is not None else None
    call('ot_ffn_fused_fwd', ctypes.byref(a), stream())
    if ev is not None:
        M = m_rows or ntiles * 128
        _probe.end('mixed_gemm', 2.0 * M * 128 * f * 2, ev, f'ffn_fused M{M} f{f} u{int(u_out is not None)}',
                   4.0 * M * 128 * 3 + 4.0 * M * f * (u_out is not None)
                   + 4.0 * M * (1 + (rstd_out is not None)), 3)


def ffn_fused_bwd_on(on: int = -1) -> int:
    """ot_ffn_fused_bwd_on: whether the block backward takes the fused FFN backward kernel where its form applies
    (split mode, hidden width 128, pair-form W2 / W1 dgrad images, float32 dU, ffn width a multiple of 128 up to
    ``FFN_FUSED_MAX_F``, the norm2 backward fused) — 1 (default), or 0: the FFN2 and FFN1 dgrad launches — or query
    (-1); returns the previous setting.  ``ONETRANS_FFN_FUSED_BWD`` sets the process's initial value."""
    return _lib.size('ot_ffn_fused_bwd_on', int(on))


def bwd_mask_fused(on: int = -1) -> int:
    """ot_bwd_mask_fused: whether the block backward, where it takes the fused FFN backward under dropout, masks dx2
    inside that kernel and inside the W2 weight gradient (1, default: no dropout pass, no dy2) or runs the dropout pass
    (0) —
    or query (-1); returns the previous setting.  ``ONETRANS_BWD_MASK_FUSED`` sets the process's initial value."""
    return _lib.size('ot_bwd_mask_fused', int(on))


def ffn_fused_bwd(dy2: Ptrish, lddy2: int, dy2_rowmax: Ptrish, dy2_rowmax_n: int, rows: Ptrish, tile_group: Ptrish,
                  ntiles: int, w2_image, w2_groups: int, w1_image, w1_groups: int, f: int, u: Ptrish, ldu: int,
                  du: Ptrish, lddu: int, x1: Ptrish, ldx1: int, gamma: Ptrish, rstd: Ptrish, dx1: Ptrish, lddx1: int,
                  dgamma: Ptrish, *, du_amax: Ptrish = None, dres: Ptrish = None, lddres: int = 0,
                  dx_masked: Ptrish = None, lddxm: int = 0, accumulate_dgamma: bool = False, amax_out: Ptrish = None,
                  rowabs_out: Ptrish = None, rowabs_n: int = 0, seed: int = 0, site: int = 0, drop: float = 0.0,
                  tail: Tuple[int, int] = (1, 1), m_rows: int = 0, device=None, mask_site: Optional[int] = None,
                  keep_out: Ptrish = None, ldkeep: int = 4) -> None:
    """ot_ffn_fused_bwd: du = (dy2 @ W2[g]^T) * gelu'(u) and dx1 = norm2_bwd(du @ W1[g]^T) + dres [, dx_masked] for
    rows of 128 floats in one launch (split mode; ``w2_image`` / ``w1_image``: the pair-form dgrad images as
    ``(tensor, element offset)``; ``dy2_rowmax``: dy2's row maxima as the FFN2 dgrad launch's ``a_rowmax``).  ``du``
    and ``du_amax`` are bit for bit that launch's; the epilogue operands are the FFN1 dgrad launch's.
    ``mask_site`` (ot_ffn_fused_bwd_mask, ``drop`` > 0): ``dy2`` is dx2, the gradient before the FFN dropout's mask at
    that site, ``dy2_rowmax`` bounds |dx2| per row, the kernel masks at fragment time and writes the rows' keep bits
    to ``keep_out`` [row][ldkeep] (int32 words)."""
    ws = workspace(size('ot_mixed_gemm_rms_workspace_size', ntiles, 128),
                   device if device is not None else (dx1[0] if isinstance(dx1, tuple) else dx1).device)
    a = _lib.FfnFusedBwdArgs(ctypes.sizeof(_lib.FfnFusedBwdArgs), ptr(dy2), lddy2, ptr(dy2_rowmax), int(dy2_rowmax_n),
                             ptr(rows), ptr(tile_group), ntiles, ptr(w2_image), int(w2_groups), ptr(w1_image),
                             int(w1_groups), f, ptr(u), ldu, ptr(du), lddu, ptr(du_amax), ptr(x1), ldx1, ptr(gamma),
                             ptr(rstd), ptr(dres), lddres, ptr(dx1), lddx1, ptr(dx_masked), lddxm, ptr(dgamma),
                             int(accumulate_dgamma), ptr(ws), ws.numel(), ptr(amax_out), ptr(rowabs_out),
                             int(rowabs_n), seed & 0xFFFFFFFF, site, float(drop), tail[0], tail[1], _sel(tail))
    ev = _probe.begin() if _probe is not None else None
    if mask_site is not None:
        call('ot_ffn_fused_bwd_mask', ctypes.byref(a), mask_site, ptr(keep_out), ldkeep, stream())
    else:
        call('ot_ffn_fused_bwd', ctypes.byref(a), stream())
    if ev is not None:
        M = m_rows or ntiles * 128
        # algorithmic bytes: dy2, u, x1, dres in; du, dx1, dx_masked out (13 R at f = 512 with dropout)
        _probe.end('mixed_gemm', 2.0 * M * 128 * f * 2, ev, f'ffn_fused_bwd M{M} f{f} drop{int(drop > 0)}',
                   4.0 * M * 128 * (3 + (dres is not None) + (dx_masked is not None)) + 4.0 * M * f * 2
                   + 4.0 * M * (1 + dy2_rowmax_n), 3)


def image_build(on: int = -1) -> int:
    """ot_image_build: whether ``split_images`` is the one-launch build, one workgroup per (bank, g, column tile)
    (1, default), or the two launches with one workgroup per unit (0: the tests' reference; same image bytes) — or
    query (-1); returns the previous setting.  ``ONETRANS_IMAGE_BUILD`` sets the process's initial value."""
    return _lib.size('ot_image_build', int(on))


def split_images(base, desc_dev, ndesc, total_units, img) -> None:
    call('ot_split_images', ptr(base), ptr(desc_dev), ndesc, total_units, ptr(img), _prec(), stream())


def attn_fwd(qkv: torch.Tensor, ld: int, B: int, H: int, I: int, K: int, hd: int, out: torch.Tensor,
             lse: torch.Tensor, qpos: Optional[torch.Tensor] = None, fp8: bool = False,
             dequant: bool = False, fp8_terms: int = 1, deq16: Optional[torch.Tensor] = None,
             amax: Optional[torch.Tensor] = None, rowmax: Optional[torch.Tensor] = None) -> None:
    """ot_attn_fwd, or with ``fp8`` (head_dim 64/128) ot_attn_fwd_fp8_ex: QK^T and PV on block-scaled fp8
    MFMA, operands as one e4m3 term or two (``fp8_terms`` 2: hi + lo, OT_FP8_TWO_TERM); ``dequant``
    (training) also overwrites qkv's operands with their dequantised fp8 values (OT_FP8_DEQUANT) for the
    backward — or, given ``deq16`` (int16 [rows, ld]: bf16 bits), writes them rounded to bf16 there
    (ot_attn_fwd_fp8_deq16; qkv is then only read)."""
    if fp8 and fp8_terms not in (1, 2):
        raise ValueError(f'fp8_terms {fp8_terms}: 1 or 2')
    ws = None
    if fp8:
        ws = workspace(size('ot_attn_fwd_fp8_workspace_size', B, H, I, hd), qkv.device)
    ev = _probe.begin() if _probe is not None else None
    if fp8 and deq16 is not None:
        call('ot_attn_fwd_fp8_deq16', ptr(qkv), ld, B, H, I, K, ptr(qpos), hd, ptr(out), ptr(lse), ptr(ws),
             ws.numel(), _lib.OT_FP8_TWO_TERM if fp8_terms == 2 else 0, ptr(deq16), stream())
    elif fp8:
        call('ot_attn_fwd_fp8_ex', ptr(qkv), ld, B, H, I, K, ptr(qpos), hd, ptr(out), ptr(lse), ptr(ws),
             ws.numel(), (_lib.OT_FP8_DEQUANT if dequant else 0) | (_lib.OT_FP8_TWO_TERM if fp8_terms == 2 else 0),
             stream())
    elif amax is not None or rowmax is not None:   # + max |O| (amax) / per (row, head) (rowmax [B*K][H])
        call('ot_attn_fwd_amax', ptr(qkv), ld, B, H, I, K, ptr(qpos), hd, ptr(out), ptr(lse), ptr(amax), ptr(rowmax),
             _prec(), stream())
    else:
        call('ot_attn_fwd', ptr(qkv), ld, B, H, I, K, ptr(qpos), hd, ptr(out), ptr(lse), _prec(), stream())
    if ev is not None:
        _probe.end('attention', 4.0 * (K * I - K * (K - 1) / 2) * hd * H * B, ev,
                   f'fwd{"_fp8" if fp8 else ""} I{I} K{K} hd{hd}')


def attn_bwd_bf16_forms(I, K, hd, qpos=None) -> int:
    """ot_attn_bwd_bf16_forms: the OT_ATTN_*_BF16 flags the backward supports at this shape."""
    return int(_lib.load().ot_attn_bwd_bf16_forms(I, K, hd, int(qpos is not None), _prec()))


def attn_bwd_bf16_supported(I, K, hd, qpos=None) -> bool:
    """ot_attn_bwd_dqkv_bf16_supported: can the backward emit dqkv in bf16 (key-grouped bf16 kernel)?"""
    return bool(_lib.load().ot_attn_bwd_dqkv_bf16_supported(I, K, hd, int(qpos is not None), _prec()))


def attn_amax_supported(I, K, hd, qpos=None, backward: bool = False) -> bool:
    """ot_attn_amax_supported: does the attention forward (or ``backward``) report max |O| (max |dQKV|) at this shape
    (the slice kernels)?"""
    return bool(_lib.load().ot_attn_amax_supported(I, K, hd, int(qpos is not None), _prec()) & (2 if backward else 1))


def attn_bwd(qkv, ld, out, dout, lse, B, H, I, K, hd, dqkv, qpos=None, dq_part_bf16: bool = False,
             amax=None, rowmax=None) -> None:
    """dqkv float32, or int16 (bf16 bits: OT_ATTN_DQKV_BF16, see attn_bwd_bf16_supported); qkv likewise
    (int16: OT_ATTN_QKV_BF16, the fp8 forward's bf16 dequantised operands)."""
    flags = ((_lib.OT_ATTN_DQKV_BF16 if dqkv.dtype == torch.int16 else 0)
             | (_lib.OT_ATTN_QKV_BF16 if qkv.dtype == torch.int16 else 0)
             | (_lib.OT_ATTN_DQ_PART_BF16 if dq_part_bf16 and dqkv.dtype == torch.int16
                and attn_bwd_bf16_forms(I, K, hd, qpos) & _lib.OT_ATTN_DQ_PART_BF16 else 0))
    ws = workspace(size('ot_attn_bwd_flags_workspace_size', B, H, I, K, hd, int(qpos is not None), flags, _prec()),
                   qkv.device)
    ev = _probe.begin() if _probe is not None else None
    if amax is not None or rowmax is not None:   # + max |dQKV| (amax) / per (row, part, head) (rowmax [B*I][3][H])
        call('ot_attn_bwd_amax', ptr(qkv), ld, ptr(out), ptr(dout), ptr(lse), B, H, I, K, ptr(qpos), hd, ptr(dqkv),
             ptr(ws), ws.numel(), ptr(amax), ptr(rowmax), _prec(), stream())
    else:
        call('ot_attn_bwd_flags', ptr(qkv), ld, ptr(out), ptr(dout), ptr(lse), B, H, I, K, ptr(qpos), hd,
             ptr(dqkv), flags, ptr(ws), ws.numel(), _prec(), stream())
    if ev is not None:
        _probe.end('attention', 8.0 * (K * I - K * (K - 1) / 2) * hd * H * B, ev, f'bwd I{I} K{K} hd{hd}')


def last_fold(on: int = -1) -> int:
    """ot_last_fold: whether the last block (one query per sample) takes the folded attention where its gate holds
    (model._fold_gate) — 1 (default; ONETRANS_LAST_FOLD) or 0: the K/V projection of every row and ot_attn_fwd — or
    query (-1); returns the previous setting."""
    return _lib.size('ot_last_fold', int(on))


def attn_fold_supported(d: int, H: int) -> bool:
    return bool(_lib.size('ot_attn_fold_supported', int(d), int(H)))


def attn_fold_rows(I: int, ded0: int, ded1: int) -> int:
    """Rows per sample of the fold backward's compact dqkv: the dedicated positions [ded0, ded1) plus the query."""
    return _lib.size('ot_attn_fold_rows', int(I), int(ded0), int(ded1))


def _fold_common(x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, hd, ded):
    return (ptr(x), ldx, ptr(rstd), ptr(gamma), ptr(w), ldw, ptr(wT), ldwT, ptr(qkv), ldqkv, B, H, I, hd, ded[0],
            ded[1])


def attn_fold_fwd(x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, hd, ded, o, lse, y) -> None:
    """ot_attn_fold_fwd: the one-query attention of the last layer on the raw rows of the shared-weight keys;
    ``ded`` = (first, end) of the dedicated key positions.  Writes o [B, d], lse [B, H], y [B, H, d]."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fold_fwd', *_fold_common(x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, hd, ded),
         ptr(o), ptr(lse), ptr(y), stream())
    if ev is not None:
        d = H * hd
        _probe.end('attention', 4.0 * I * d * H * B, ev, f'fold_fwd I{I} hd{hd}', 4.0 * B * I * (d + 1))


def attn_fold_bwd(x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, hd, ded, o, dout, lse, y, dx1, dx, lddx,
                  dqkv, lddqkv, z, dgpart) -> None:
    """ot_attn_fold_bwd: dx of every row of the layer input (through its use as a key; zero for a dedicated row,
    + dx1 on the query row), the compact dqkv rows of the dedicated keys and the query, z and the dgamma parts."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fold_bwd', *_fold_common(x, ldx, rstd, gamma, w, ldw, wT, ldwT, qkv, ldqkv, B, H, I, hd, ded),
         ptr(o), ptr(dout), ptr(lse), ptr(y), ptr(dx1), ptr(dx), lddx, ptr(dqkv), lddqkv, ptr(z), ptr(dgpart),
         stream())
    if ev is not None:
        d = H * hd
        _probe.end('attention', 10.0 * I * d * H * B, ev, f'fold_bwd I{I} hd{hd}', 8.0 * B * I * (d + 1))


def attn_fold_dw(z, y, qkv, ldqkv, dout, gamma, B, H, I, hd, dW, lddw, accumulate: bool = False) -> None:
    """ot_attn_fold_dw: group 0's dWk / dWv blocks from z / y and q / dout (fixed-order partial sums)."""
    ws = workspace(size('ot_attn_fold_workspace_size', B, H * hd), z.device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fold_dw', ptr(z), ptr(y), ptr(qkv), ldqkv, ptr(dout), ptr(gamma), B, H, I, hd, ptr(dW), lddw,
         int(accumulate), ptr(ws), ws.numel(), stream())
    if ev is not None:
        d = H * hd
        _probe.end('attention', 4.0 * B * d * d, ev, f'fold_dw B{B}', 8.0 * B * d * (H + 1))


def attn_fold_dgamma(dgpart, B, d, dgamma, accumulate: bool = False) -> None:
    """ot_attn_fold_dgamma: dgamma (+)= the samples' parts, summed in a fixed order."""
    ws = workspace(size('ot_attn_fold_workspace_size', B, d), dgpart.device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fold_dgamma', ptr(dgpart), B, d, ptr(dgamma), int(accumulate), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('attention', 0.0, ev, f'fold_dgamma B{B}', 4.0 * B * d)


def _valid_arg(valid):
    """A key-padding mask argument (uint8 tensor, element offset, row stride) as (pointer, stride)."""
    t, off, ldv = valid
    if t.dtype != torch.uint8:
        raise TypeError(f'key_valid: uint8 expected, got {t.dtype}')
    return ptr((t, off)), ldv


def attn_fwd_masked(qkv, ld, B, H, I, K, hd, out, lse, key_valid, qpos=None) -> None:
    """ot_attn_fwd_masked: ot_attn_fwd under a key-padding mask.  ``key_valid`` = (uint8 tensor, element offset, row
    stride): sample b's I bytes start at offset + b * stride (a layer's slice of layer 0's array)."""
    kv, ldv = _valid_arg(key_valid)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fwd_masked', ptr(qkv), ld, B, H, I, K, ptr(qpos), hd, kv, ldv, ptr(out), ptr(lse), _prec(),
         stream())
    if ev is not None:
        _probe.end('attention', 4.0 * (K * I - K * (K - 1) / 2) * hd * H * B, ev, f'fwd_masked I{I} K{K} hd{hd}')


def attn_bwd_masked(qkv, ld, out, dout, lse, B, H, I, K, hd, dqkv, key_valid, qpos=None) -> None:
    """ot_attn_bwd_masked: ot_attn_bwd under the forward's key-padding mask (float32 dqkv)."""
    kv, ldv = _valid_arg(key_valid)
    ws = workspace(size('ot_attn_bwd_workspace_size', B, H, K), qkv.device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_bwd_masked', ptr(qkv), ld, ptr(out), ptr(dout), ptr(lse), B, H, I, K, ptr(qpos), hd, kv, ldv,
         ptr(dqkv), ptr(ws), _prec(), stream())
    if ev is not None:
        _probe.end('attention', 8.0 * (K * I - K * (K - 1) / 2) * hd * H * B, ev, f'bwd_masked I{I} K{K} hd{hd}')


def attn_fwd_cached_masked(qkv, ld, kv_cache, ldc, req, C, H, Ic, n, Kq, hd, out, cache_valid, lse=None) -> None:
    """ot_attn_fwd_cached_masked: ot_attn_fwd_cached (with ``lse``: ot_attn_fwd_cached_lse) with a key-padding mask
    over the cached rows, ``cache_valid`` = (uint8 tensor, element offset, row stride) or None when Ic == 0."""
    cv, ldcv = _valid_arg(cache_valid) if cache_valid is not None else (None, 0)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fwd_cached_masked', ptr(qkv), ld, ptr(kv_cache), ldc, ptr(req), C, H, Ic, n, Kq, hd, cv, ldcv,
         ptr(out), ptr(lse), stream())
    if ev is not None:
        _probe.end('attention', 4.0 * (Kq * (Ic + n) - Kq * (Kq - 1) / 2) * hd * H * C, ev,
                   f'fwd_cached_masked Ic{Ic} n{n} K{Kq} hd{hd}')


def kv_pack_bf16(qkv, ld, R, rows_per_req, d, kv16, ldc16, req_stride, row0) -> None:
    """ot_kv_pack_bf16: the K | V columns of ``qkv``'s R * rows_per_req rows, rounded to bf16, into rows
    row0 .. row0 + rows_per_req - 1 of every request of the bf16 cache ``kv16`` (req_stride rows of ldc16 each)."""
    if kv16.dtype != torch.bfloat16:
        raise TypeError(f'kv_pack_bf16: a bfloat16 cache is expected, got {kv16.dtype}')
    ev = _probe.begin() if _probe is not None else None
    call('ot_kv_pack_bf16', ptr(qkv), ld, R, rows_per_req, d, ptr(kv16), ldc16, req_stride, row0, stream())
    if ev is not None:
        _probe.end('rowwise', 0.0, ev, f'kv_pack_bf16 R{R} rows{rows_per_req} d{d}')


def attn_fwd_cached_kv16(qkv, ld, kv16, ldc16, req_stride, req, C, H, Ic, n, Kq, hd, out, cache_valid=None,
                         lse=None) -> None:
    """ot_attn_fwd_cached_kv16: ot_attn_fwd_cached_masked over a bf16 cache (request r's key j = row
    r * req_stride + j of ``kv16``, K at col 0, V at col d); ``cache_valid`` None = every cached row valid."""
    if kv16 is not None and kv16.dtype != torch.bfloat16:
        raise TypeError(f'attn_fwd_cached_kv16: a bfloat16 cache is expected, got {kv16.dtype}')
    cv, ldcv = _valid_arg(cache_valid) if cache_valid is not None else (None, 0)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_fwd_cached_kv16', ptr(qkv), ld, ptr(kv16), ldc16, req_stride, ptr(req), C, H, Ic, n, Kq, hd, cv,
         ldcv, ptr(out), ptr(lse), stream())
    if ev is not None:
        _probe.end('attention', 4.0 * (Kq * (Ic + n) - Kq * (Kq - 1) / 2) * hd * H * C, ev,
                   f'fwd_cached_kv16 Ic{Ic} n{n} K{Kq} hd{hd}')


def seq_key_valid(lens, seq_len, seq_off, B: int, L0: int, valid0, rank=None) -> None:
    """ot_seq_key_valid: layer 0's key-padding mask valid0 [B, L0] (uint8) from the present sequences' lengths
    ``lens`` (device int32 [nseq, B]), their caps ``seq_len`` and first token positions ``seq_off`` (host ints), and
    under time fusion the events' ranks ``rank`` [B, L_S] (seq_time_rows' rank_out)."""
    n = len(seq_len)
    arr = ctypes.c_int32 * max(1, n)
    sl, so = arr(*seq_len), arr(*seq_off)               # (read by the call itself: host descriptors)
    call('ot_seq_key_valid', ptr(lens), ctypes.cast(sl, ctypes.c_void_p), ctypes.cast(so, ctypes.c_void_p), n, B, L0,
         ptr(rank),
         rank.shape[1] if rank is not None else 0, ptr(valid0), stream())


def attn_fwd_cached(qkv, ld, kv_cache, ldc, req, C, H, Ic, n, Kq, hd, out, lse=None) -> None:
    """ot_attn_fwd_cached: N-side queries over a request's cached S-side K/V plus their own rows; given ``lse``
    [C, H, Kq], ot_attn_fwd_cached_lse: the same forward, which also writes lse for the backward."""
    ev = _probe.begin() if _probe is not None else None
    args = (ptr(qkv), ld, ptr(kv_cache), ldc, ptr(req), C, H, Ic, n, Kq, hd, ptr(out))
    if lse is None:
        call('ot_attn_fwd_cached', *args, stream())
    else:
        call('ot_attn_fwd_cached_lse', *args, ptr(lse), stream())
    if ev is not None:
        _probe.end('attention', 4.0 * (Kq * (Ic + n) - Kq * (Kq - 1) / 2) * hd * H * C, ev,
                   f'fwd_cached{"" if lse is None else "_lse"} Ic{Ic} n{n} K{Kq} hd{hd}')


attn_fwd_cached_lse = attn_fwd_cached    # the name tests/test_request_attn_gpu.py calls the lse form by


def attn_bwd_cached(qkv, ld, kv_cache, ldc, req_start, R, C, H, Ic, n, Kq, hd, out, dout, lse, dqkv, dkv_cache,
                    accumulate: bool = False) -> None:
    """ot_attn_bwd_cached: dq / dk / dv of the candidates' rows into dqkv, the cached rows' dK / dV (summed over a
    request's candidates, deterministic) into dkv_cache (written, or added to with ``accumulate``)."""
    ws = workspace(size('ot_attn_bwd_cached_workspace_size', R, C, H, Ic, n, Kq, hd), qkv.device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_attn_bwd_cached', ptr(qkv), ld, ptr(kv_cache), ldc, ptr(req_start), R, C, H, Ic, n, Kq, hd, ptr(out),
         ptr(dout), ptr(lse), ptr(dqkv), ptr(dkv_cache), int(bool(accumulate)), ptr(ws), ws.numel(), stream())
    if ev is not None:
        # own rows once; the cached part's S / dP are formed twice (dK/dV pass and the recomputing dQ pass)
        _probe.end('attention', (8.0 * (Kq * n - Kq * (Kq - 1) / 2) + 14.0 * Kq * Ic) * hd * H * C, ev,
                   f'bwd_cached Ic{Ic} n{n} K{Kq} hd{hd}')


def rmsnorm_fwd(x: Ptrish, ldx: int, rows: int, d: int, rstd: Ptrish, gamma: Ptrish = None, y: Ptrish = None,
                ldy: int = 0, eps: float = 1e-6) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_rmsnorm_fwd', ptr(x), ldx, ptr(gamma), ptr(y), ldy, ptr(rstd), rows, d, eps, stream())
    if ev is not None:
        _probe.end('rowwise', 0.0, ev)


def rmsnorm_bwd(dy: Ptrish, lddy: int, x: Ptrish, ldx: int, gamma: Ptrish, rstd: Ptrish, dx: Ptrish, lddx: int,
                rows: int, d: int, *, dres: Ptrish = None, lddres: int = 0, dres_tail=(0, 0), dx_masked: Ptrish = None,
                lddxm: int = 0, seed: int = 0, site: int = 0, drop: float = 0.0, tail=(1, 1),
                dgamma: Ptrish = None, accumulate: bool = False, device=None) -> None:
    nbytes = size('ot_rmsnorm_bwd_workspace_size', rows, d) if dgamma is not None else 16
    ws = workspace(nbytes, device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_rmsnorm_bwd', ptr(dy), lddy, ptr(x), ldx, ptr(gamma), ptr(rstd), ptr(dres), lddres, dres_tail[0],
         dres_tail[1], _sel(dres_tail), ptr(dx), lddx, ptr(dx_masked), lddxm, seed & 0xFFFFFFFF, site, float(drop),
         tail[0], tail[1], _sel(tail), ptr(dgamma), int(accumulate), rows, d, ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('rowwise', 0.0, ev)


def dropout_apply(src, lds, dst, ldd, rows, d, seed, site, drop, tail, amax=None, rowmax=None) -> None:
    """dst float32, or int16 (bf16 bits: ot_dropout_apply_bf16).  ``amax`` (one float, zeroed) / ``rowmax`` ([rows][ceil(d /
    256)]): the output's magnitude for fp16-pair consumers (ot_dropout_apply_ex, float32 dst)."""
    ev = _probe.begin() if _probe is not None else None
    if amax is not None or rowmax is not None:
        call('ot_dropout_apply_ex', ptr(src), lds, ptr(dst), ldd, rows, d, seed & 0xFFFFFFFF, site, float(drop),
             tail[0], tail[1], _sel(tail), ptr(amax), ptr(rowmax), (d + 255) // 256 if rowmax is not None else 0,
             stream())
    else:
        fn = 'ot_dropout_apply_bf16' if getattr(dst, 'dtype', None) == torch.int16 else 'ot_dropout_apply'
        call(fn, ptr(src), lds, ptr(dst), ldd, rows, d, seed & 0xFFFFFFFF, site, float(drop), tail[0],
             tail[1], _sel(tail), stream())
    if ev is not None:
        _probe.end('rowwise', 0.0, ev, 'dropout_apply')


def dropout_rowmax_supported(d: int) -> bool:
    """ot_dropout_rowmax_supported: does ``dropout_apply`` report ``rowmax`` at this row width?"""
    return bool(_lib.load().ot_dropout_rowmax_supported(d))


def rows_absmax(x, ldx, rows, d, out) -> None:
    """ot_rows_absmax: out [rows][ceil(d / 256)] = each row's 256-column parts' max |x| (an fp16-pair GEMM's a_rowmax)."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_rows_absmax', ptr(x), ldx, rows, d, ptr(out), (d + 255) // 256, stream())
    if ev is not None:
        _probe.end('rowwise', 0.0, ev, 'rows_absmax')


def pair_split_probe(x: torch.Tensor, scale: float, form: str = 'pair8'):
    """ot_pair_split_probe: the (hi, lo) fp16 planes, as int16 bit patterns, that the pair GEMMs form from the flat
    f32 tensor ``x`` at ``scale``; ``form`` 'pair8' (saturating; numel a multiple of 8), 'pair4' (the weight gradient's)
    or 'slice' (the slice attention's; both: numel a multiple of 4)."""
    hi = torch.empty(x.numel(), dtype=torch.int16, device=x.device)
    lo = torch.empty_like(hi)
    call('ot_pair_split_probe', ptr(x), x.numel(), float(scale), {'pair8': 0, 'pair4': 1, 'slice': 2}[form], ptr(hi), ptr(lo),
         stream())
    return hi, lo


def rows_colsum(src, ld, rows: Ptrish, nrows: int, ncols: int, out: Ptrish, accumulate=False, device=None) -> None:
    ws = workspace(size('ot_rows_colsum_workspace_size', nrows, ncols), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_rows_colsum', ptr(src), ld, ptr(rows), nrows, ncols, ptr(out), int(accumulate), ptr(ws), ws.numel(),
         stream())
    if ev is not None:
        _probe.end('rowwise', 0.0, ev)


def ns_assemble(fields_dev, nfields, table, B, out, ld_out) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_assemble', ptr(fields_dev), nfields, ptr(table), B, ptr(out), ld_out, stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def ns_grad_pack(fields_dev, nsparse, width, dmat, ld, B, keys, grads) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_grad_pack', ptr(fields_dev), nsparse, width, ptr(dmat), ld, B, ptr(keys), ptr(grads), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def fill_rows(dst, ld, rows, nrows, vec, d) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_fill_rows', ptr(dst), ld, ptr(rows), nrows, ptr(vec), d, stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def seq_rows(ids, stride_b, B, L, vocab, in_rows) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_seq_rows', ptr(ids), stride_b, B, L, vocab, ptr(in_rows), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def head_fwd(pre1, w2, b2, T, B, dh, logits, probs) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_head_fwd', ptr(pre1), ptr(w2), ptr(b2), T, B, dh, ptr(logits), ptr(probs), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def head_bwd(pre1, w2, probs, dprobs, T, B, dh, dpre1, dw2, db2, sw2, sb2, accumulate=False, device=None,
             dlogits=None) -> None:
    """ot_head_bwd_ex: the loss gradient w.r.t. the probabilities (``dprobs``) and / or the logits."""
    ws = workspace(size('ot_head_bwd_workspace_size', T, B, dh), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_head_bwd_ex', ptr(pre1), ptr(w2), ptr(probs), ptr(dprobs), ptr(dlogits), T, B, dh, ptr(dpre1), ptr(dw2),
         ptr(db2), sw2, sb2, int(accumulate), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def bce_fwd(probs, labels, T, B, loss, device=None, mse_mask: int = 0) -> None:
    """Σ_task loss (train.py:78-93): BCE, or MSE for the tasks whose bit is set in ``mse_mask``."""
    ws = workspace(size('ot_bce_workspace_size', T, B), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_task_loss_fwd', ptr(probs), ptr(labels), T, B, mse_mask, ptr(loss), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def bce_bwd(probs, labels, gscale, T, B, dprobs, mse_mask: int = 0) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_task_loss_bwd', ptr(probs), ptr(labels), ptr(gscale), T, B, mse_mask, ptr(dprobs), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def metrics_update(probs, labels, T, B, task_stride, bounds, nb, counts, sums, device=None) -> None:
    """Streaming metric state += this batch (train.py:140-150): ``counts`` [T, 2, nb+1] int64 (class x bin
    over the ``nb`` ascending float64 ``bounds``), ``sums`` [T, 4] float64 {n, Σ(p-y)², Σ|p-y|, Σ bce}."""
    ws = workspace(size('ot_metrics_workspace_size', T, B), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_metrics_update', ptr(probs), ptr(labels), T, B, task_stride, ptr(bounds), nb, ptr(counts), ptr(sums),
         ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('metrics', 0.0, ev)


def metrics_update_weighted(probs, labels, weights, T, B, task_stride, weight_stride, bounds, nb, counts, sums,
                            device=None) -> None:
    """``metrics_update`` under per-sample weights (Keras metrics with ``sample_weight``): task t's weights at
    ``weights + t * weight_stride`` (0: one [B] row for all tasks).  The state is then in units of 2^-24
    (``_lib.OT_METRICS_WEIGHT_ONE`` per unit weight); a zero weight skips the sample."""
    ws = workspace(size('ot_metrics_weighted_workspace_size', T, B), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_metrics_update_weighted', ptr(probs), ptr(labels), ptr(weights), T, B, task_stride, weight_stride,
         ptr(bounds), nb, ptr(counts), ptr(sums), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('metrics', 0.0, ev)


def grouped_auc(groups, scores, labels, T, n, task_stride, group_bits, task_mask, agg, num_groups, group_ids=None,
                group_stats=None, device=None) -> None:
    """ot_grouped_auc over ``n`` records: ``agg`` [T, 4] float64 {Σ n_u·AUC_u, Σ AUC_u, Σ n_u, #valid groups},
    ``num_groups`` [1] int64; optionally the distinct ids [n] and the per-group {n_pos, n_neg, 2U} [T, n, 3]."""
    ws = workspace(size('ot_grouped_auc_workspace_size', T, n, group_bits), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_grouped_auc', ptr(groups), ptr(scores), ptr(labels), T, n, task_stride, group_bits, task_mask, ptr(agg),
         ptr(num_groups), ptr(group_ids), ptr(group_stats), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('grouped_auc', 0.0, ev)


def rank_topk(probs, task_stride, T, weights, mode, req, C, R, K, top_idx, top_score, count, fused_out=None,
              device=None) -> None:
    """ot_rank_topk: per request the ``K`` best of its candidates under the fused score (``mode`` 'sum':
    Σ w_t p_t by fma in task order; 'product': Π p_t over w_t != 0), ties to the lower candidate index.
    ``probs`` task-major with ``task_stride``, ``weights`` T host floats (passed by value, no device copy),
    ``req`` [C] int32 (outside [0, R): excluded).  Writes ``top_idx`` [R, K] int32 (-1 padded), ``top_score``
    [R, K] f32 (-inf padded), ``count`` [R] int32 and optionally ``fused_out`` [C]."""
    if mode not in _lib.RANK_MODES:
        raise ValueError(f'rank mode {mode!r}: expected one of {sorted(_lib.RANK_MODES)}')
    if len(weights) != T:
        raise ValueError(f'rank_topk: {len(weights)} weights for {T} tasks')
    wts = (ctypes.c_float * max(T, 1))(*[float(w) for w in weights])
    ws = workspace(size('ot_rank_topk_workspace_size', R, C, K), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_rank_topk', ptr(probs), task_stride, T, wts, _lib.RANK_MODES[mode], ptr(req), C, R, K, ptr(top_idx),
         ptr(top_score), ptr(count), ptr(fused_out), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('rank', 0.0, ev)


def ns_bag_descs(bags):
    """The host descriptor array of ``ns_bag_pool`` / ``ns_bag_grad_pack``: ``bags`` = [dict(table, ids, weights,
    row_offset, num_rows, ids_stride, weights_stride, width, cap, col, pooling)] with device tensors (or None for
    ``weights``) and ``pooling`` 'sum' | 'mean'.  Build it once for buffers that persist (OneTransModel's plan)."""
    arr = (_lib.NsBag * max(1, len(bags)))()
    for k, b in enumerate(bags):
        arr[k] = _lib.NsBag(ptr(b['table']), ptr(b['ids']), ptr(b.get('weights')), int(b['row_offset']),
                            int(b['num_rows']), int(b['ids_stride']), int(b.get('weights_stride', 0)),
                            int(b['width']), int(b['cap']), int(b['col']), _lib.BAG_POOLINGS[b['pooling']])
    return arr


def _bag_slice(descs, first: int, nbags: int):
    return ctypes.cast(ctypes.byref(descs, first * ctypes.sizeof(_lib.NsBag)), ctypes.c_void_p) if nbags else None


def ns_bag_pool(descs, nbags: int, B: int, out, ld_out: int, coef_out, first: int = 0) -> None:
    """ot_ns_bag_pool over ``descs[first : first + nbags]``: each bag's pooled rows into its columns of ``out``
    [B, ld_out]; ``coef_out`` (f32, sum of B * cap) receives the per-slot coefficients the backward reads."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_bag_pool', _bag_slice(descs, first, nbags), nbags, B, ptr(out), ld_out, ptr(coef_out), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def ns_bag_grad_pack(descs, nbags: int, B: int, dmat, ld: int, coef, keys, grads, first: int = 0) -> None:
    """ot_ns_bag_grad_pack over ``descs[first : first + nbags]`` (the bags of one table): keys (int64) and gradient
    rows of every slot, bag-major; ``coef`` is the pool's ``coef_out`` at bag ``first``'s base."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_bag_grad_pack', _bag_slice(descs, first, nbags), nbags, B, ptr(dmat), ld, ptr(coef), ptr(keys),
         ptr(grads), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def ns_group_fwd(A: Ptrish, lda: int, goff: Ptrish, G: int, ktot: int, kmax: int, W: Ptrish, bias: Ptrish, B: int,
                 d: int, X: Ptrish, ldx: int) -> None:
    """ot_ns_group_fwd: NS token g of row b = A[b, goff[g]:goff[g+1]] @ W[goff[g]:goff[g+1]] + bias[g] (exact f32).
    ``goff``: device int32 [G+1]; ``ktot`` = goff[G], ``kmax`` >= the widest group."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_group_fwd', ptr(A), lda, ptr(goff), G, ktot, kmax, ptr(W), ptr(bias), B, d, ptr(X), ldx, stream())
    if ev is not None:
        _probe.end('mixed_gemm', 2.0 * B * ktot * d, ev, f'ns_group_fwd M{B} K{ktot} N{d} G{G}',
                   4.0 * (B * ktot + ktot * d + B * G * d))


def ns_group_bwd_input(D: Ptrish, ldd: int, goff: Ptrish, G: int, ktot: int, kmax: int, W: Ptrish, B: int, d: int,
                       dA: Ptrish, lda: int) -> None:
    """ot_ns_group_bwd_input: dA[b, goff[g]:goff[g+1]] = D[b, g] @ W[goff[g]:goff[g+1]]^T."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_group_bwd_input', ptr(D), ldd, ptr(goff), G, ktot, kmax, ptr(W), B, d, ptr(dA), lda, stream())
    if ev is not None:
        _probe.end('mixed_gemm', 2.0 * B * ktot * d, ev, f'ns_group_bwd_input M{B} K{ktot} N{d} G{G}',
                   4.0 * (B * ktot + ktot * d + B * G * d))


def ns_group_bwd_weight(A: Ptrish, lda: int, D: Ptrish, ldd: int, goff: Ptrish, G: int, ktot: int, kmax: int, B: int,
                        d: int, dW: Ptrish, db: Ptrish, accumulate: bool = False, device=None) -> None:
    """ot_ns_group_bwd_weight: dW[goff[g]:goff[g+1]] (+)= A[:, goff[g]:goff[g+1]]^T @ D[:, g], db[g] (+)= sum_b D[b, g]
    (deterministic: partial slabs per row chunk, added in chunk order)."""
    ws = workspace(size('ot_ns_group_wgrad_workspace_size', B, G, ktot, d), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_ns_group_bwd_weight', ptr(A), lda, ptr(D), ldd, ptr(goff), G, ktot, kmax, B, d, ptr(dW), ptr(db),
         int(accumulate), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('mixed_gemm', 2.0 * B * ktot * d, ev, f'ns_group_bwd_weight M{B} K{ktot} N{d} G{G}',
                   4.0 * (B * ktot + B * G * d + (ktot + G) * d))


def seq_time_descs(seqs):
    """The host descriptor array of ``seq_time_rows``: ``seqs`` = [(times, stride_b, L, map_off)], ``times`` a device
    int64 tensor (or (tensor, element offset)).  Build it once for buffers that persist (OneTransModel's plan)."""
    arr = (_lib.SeqTime * max(1, len(seqs)))()
    for k, (t, stride_b, L, off) in enumerate(seqs):
        arr[k] = _lib.SeqTime(ptr(t), int(stride_b), int(L), int(off))
    return arr


def seq_time_rows(descs, nseq: int, B: int, L_S: int, row_stride: int, out_rows, rank_out=None, last_time=None,
                  device=None) -> None:
    """ot_seq_time_rows: per sample the stable order of its L_S events by (time, sequence, position); writes
    out_rows[map_off_i + b L_i + j] = b row_stride + rank, optionally ``rank_out`` [B, L_S] int32 (concatenation
    order) and ``last_time`` [B] int64.  ``descs``: seq_time_descs(...)."""
    ws = workspace(size('ot_seq_time_rows_workspace_size', B, nseq, L_S), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_seq_time_rows', ctypes.cast(descs, ctypes.c_void_p), nseq, B, L_S, row_stride, ptr(out_rows),
         ptr(rank_out), ptr(last_time), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def task_loss_logits_fwd(logits, probs, labels, T, B, loss, device=None, mse_mask: int = 0) -> None:
    """Σ_task loss (train.py:78-93) as Keras 2.12 computes it on sigmoid heads: BCE from the logits, MSE
    (bits of ``mse_mask``) from the probabilities."""
    ws = workspace(size('ot_bce_workspace_size', T, B), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_task_loss_logits_fwd', ptr(logits), ptr(probs), ptr(labels), T, B, mse_mask, ptr(loss), ptr(ws),
         ws.numel(), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def task_loss_logits_bwd(probs, labels, gscale, T, B, dlogits, mse_mask: int = 0) -> None:
    ev = _probe.begin() if _probe is not None else None
    call('ot_task_loss_logits_bwd', ptr(probs), ptr(labels), ptr(gscale), T, B, mse_mask, ptr(dlogits), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def task_loss_weighted_fwd(logits, probs, labels, weights, weight_stride, task_scale, T, B, loss, denom, device=None,
                           mse_mask: int = 0, reduction: str = 'batch') -> None:
    """Σ_t a_t (Σ_b w l) / denom_t with l the per-element term of the un-weighted calls (``logits`` None: the
    probability form), ``denom_t`` = B ('batch') or Σ_b w ('weights').  Writes ``loss`` [1] and ``denom`` [T]."""
    ws = workspace(size('ot_task_loss_weighted_workspace_size', T, B), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_task_loss_weighted_fwd', ptr(logits), ptr(probs), ptr(labels), ptr(weights), weight_stride,
         ptr(task_scale), T, B, mse_mask, _lib.LOSS_REDUCTIONS[reduction], ptr(loss), ptr(denom), ptr(ws), ws.numel(),
         stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def task_loss_weighted_bwd(probs, labels, weights, weight_stride, task_scale, denom, gscale, T, B, dout,
                           mse_mask: int = 0, prob_form: bool = False) -> None:
    """``dout`` = gscale a_t w ∂l/∂z / denom_t (``prob_form``: ∂l/∂p), exactly 0 where the weight is 0."""
    ev = _probe.begin() if _probe is not None else None
    call('ot_task_loss_weighted_bwd', ptr(probs), ptr(labels), ptr(weights), weight_stride, ptr(task_scale),
         ptr(denom), ptr(gscale), T, B, mse_mask, int(bool(prob_form)), ptr(dout), stream())
    if ev is not None:
        _probe.end('head_loss', 0.0, ev)


def sparse_adagrad(table, accum, E, num_rows, keys, grads, n, lr, eps, clip, device=None) -> None:
    ws = workspace(size('ot_sparse_adagrad_workspace_size', n, E), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_sparse_adagrad', ptr(table), ptr(accum), E, num_rows, ptr(keys), ptr(grads), n, float(lr), float(eps),
         float(clip), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def sparse_grad_dense(E, num_rows, keys, grads, n, dense, device=None) -> None:
    """dense[key] = sum of the gradient rows of key (dense must be zero on entry)."""
    ws = workspace(size('ot_sparse_adagrad_workspace_size', n, E), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_sparse_grad_dense', E, num_rows, ptr(keys), ptr(grads), n, ptr(dense), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def dense_adagrad(table, accum, grad, num_rows, E, lr, eps, clip, device=None) -> None:
    ws = workspace(size('ot_dense_adagrad_workspace_size'), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_dense_adagrad', ptr(table), ptr(accum), ptr(grad), num_rows, E, float(lr), float(eps), float(clip),
         ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def sparse_prepare(E, num_rows, keys, grads, n, sumsq_out, ws) -> None:
    call('ot_sparse_prepare', E, num_rows, ptr(keys), ptr(grads), n, ptr(sumsq_out), ptr(ws), ws.numel(), stream())


def sparse_finish(table, accum, E, n, lr, eps, clip, sumsq_total, ws) -> None:
    call('ot_sparse_finish', ptr(table), ptr(accum), E, n, float(lr), float(eps), float(clip), ptr(sumsq_total),
         ptr(ws), ws.numel(), stream())


def sparse_adagrad_rowwise(table, accum_rows, E, num_rows, keys, grads, n, lr, eps, clip, device=None) -> None:
    """Row-wise Adagrad (``accum_rows`` [num_rows]): the one-call form."""
    ws = workspace(size('ot_sparse_adagrad_workspace_size', n, E), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_sparse_adagrad_rowwise', ptr(table), ptr(accum_rows), E, num_rows, ptr(keys), ptr(grads), n, float(lr),
         float(eps), float(clip), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def dense_adagrad_rowwise(table, accum_rows, grad, num_rows, E, lr, eps, clip, device=None) -> None:
    """Row-wise Adagrad over a dense [num_rows, E] gradient (the data-parallel form)."""
    ws = workspace(size('ot_dense_adagrad_workspace_size'), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_dense_adagrad_rowwise', ptr(table), ptr(accum_rows), ptr(grad), num_rows, E, float(lr), float(eps),
         float(clip), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('embedding', 0.0, ev)


def sparse_finish_rowwise(table, accum_rows, E, n, lr, eps, clip, sumsq_total, ws) -> None:
    """Row-wise Adagrad: the second phase after ``sparse_prepare`` (row-sharded tables)."""
    call('ot_sparse_finish_rowwise', ptr(table), ptr(accum_rows), E, n, float(lr), float(eps), float(clip),
         ptr(sumsq_total), ptr(ws), ws.numel(), stream())


def sparse_workspace(n, E, device):
    return workspace(size('ot_sparse_adagrad_workspace_size', n, E), device)


def shard_route(ids, n, num_rows, world, perm, send_local, counts) -> None:
    ws = workspace(size('ot_shard_route_workspace_size', n), ids.device)
    call('ot_shard_route', ptr(ids), n, num_rows, world, ptr(perm), ptr(send_local), ptr(counts), ptr(ws), ws.numel(),
         stream())


def shard_route_unique(ids, n, num_rows, world, uniq_local, inv, order, run_start, counts) -> None:
    ws = workspace(size('ot_shard_route_unique_workspace_size', n), ids.device)
    call('ot_shard_route_unique', ptr(ids), n, num_rows, world, ptr(uniq_local), ptr(inv), ptr(order), ptr(run_start),
         ptr(counts), ptr(ws), ws.numel(), stream())


def segment_rows_sum(src, order, run_start, U, E, out, n: Optional[int] = None) -> None:
    """Per distinct id the sum of its repeats' rows (ot_segment_rows_sum_ex: hot runs split into pieces);
    ``n`` = the routed id count (run_start[U]; default: src's rows)."""
    n = int(src.shape[0]) if n is None else int(n)
    n = max(n, int(U))
    ws = workspace(size('ot_segment_rows_sum_workspace_size', U, n, E), src.device)
    call('ot_segment_rows_sum_ex', ptr(src), ptr(order), ptr(run_start), U, n, E, ptr(out), ptr(ws), ws.numel(),
         stream())


def gather_rows(table, E, idx, n, out) -> None:
    call('ot_gather_rows', ptr(table), E, ptr(idx), n, ptr(out), stream())


def permute_rows(src, perm, n, E, inverse, dst) -> None:
    call('ot_permute_rows', ptr(src), ptr(perm), n, E, int(inverse), ptr(dst), stream())


def hash_uniform_rows(out, local_rows, E, rank, world, seed, lo, hi) -> None:
    call('ot_hash_uniform_rows', ptr(out), local_rows, E, rank, world, seed & 0xFFFFFFFF, float(lo), float(hi),
         stream())


def clip_rmsprop(w, g, v, m, segs_dev, nseg, max_seg, lr, rho, eps, momentum, clip, device=None) -> None:
    ws = workspace(size('ot_clip_rmsprop_workspace_size', nseg, max_seg), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_clip_rmsprop', ptr(w), ptr(g), ptr(v), ptr(m), ptr(segs_dev), nseg, max_seg, float(lr), float(rho),
         float(eps), float(momentum), float(clip), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('optimizer', 0.0, ev)


def clip_adam(w, g, m, v, segs_dev, nseg, max_seg, lr, beta1, beta2, eps, step, clip, device=None) -> None:
    """Per-segment clip + Keras Adam (ot_clip_adam); ``step`` is the 1-based index of the step being applied."""
    ws = workspace(size('ot_clip_adam_workspace_size', nseg, max_seg), device)
    ev = _probe.begin() if _probe is not None else None
    call('ot_clip_adam', ptr(w), ptr(g), ptr(m), ptr(v), ptr(segs_dev), nseg, max_seg, float(lr), float(beta1),
         float(beta2), float(eps), int(step), float(clip), ptr(ws), ws.numel(), stream())
    if ev is not None:
        _probe.end('optimizer', 0.0, ev)
