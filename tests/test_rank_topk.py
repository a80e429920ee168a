"""CPU: the ranking yardstick (tests/rank_ref.py) against hand-written cases, and the host side of
ot_rank_topk: exported symbols, header/ctypes agreement, workspace sizing, argument validation."""

import os
import re

import numpy as np
import pytest

from recommend_amd import _lib

import rank_ref as RR

NAN, INF = np.float32(np.nan), np.float32(np.inf)
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')


def _rank(f, req, R, K):
    idx, score, count = RR.rank_topk(np.array(f, np.float32), req, R, K)
    return idx.tolist(), score, count.tolist()


def test_ref_ties_go_to_the_lower_index():
    #        c: 0    1    2    3    4    5    6
    idx, score, count = _rank([0.5, 0.9, 0.5, 0.9, 0.1, 0.5, 0.9], [0] * 7, 1, 5)
    assert idx == [[1, 3, 6, 0, 2]] and count == [5]
    assert score[0].tolist() == [np.float32(0.9)] * 3 + [np.float32(0.5)] * 2


def test_ref_nan_ranks_below_minus_inf():
    idx, score, count = _rank([NAN, -INF, 0.25, NAN, -3.0, INF], [0] * 6, 1, 6)
    assert idx == [[5, 2, 4, 1, 0, 3]] and count == [6]
    assert np.isnan(score[0, 4:]).all() and score[0, 3] == -INF
    idx, _, _ = _rank([NAN, -INF, 0.25, NAN, -3.0, INF], [0] * 6, 1, 4)      # the NaNs are not needed
    assert idx == [[5, 2, 4, 1]]


def test_ref_minus_zero_ties_with_zero():
    #        c: 0     1    2     3    4     5
    idx, score, _ = _rank([-0.0, 0.0, -1.0, 0.0, 1e-45, -0.0], [0] * 6, 1, 6)
    assert idx == [[4, 0, 1, 3, 5, 2]]                    # the zeros in index order, whatever their sign
    assert RR.bits(score[0, 1:5]).tolist() == [0x80000000, 0, 0, 0x80000000]  # and returned bit for bit


def test_ref_infinities():
    idx, score, _ = _rank([1.0, INF, -INF, 3e38, INF, -3e38, 0.0], [0] * 7, 1, 7)
    assert idx == [[1, 4, 3, 0, 6, 5, 2]]
    assert score[0, 0] == INF and score[0, 6] == -INF


def test_ref_exclusion_and_padding():
    #              c: 0    1    2    3    4    5    6    7
    f = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
    req = [1, -1, 0, 3, 1, 0, -7, 1]                     # R = 3: -1, 3 and -7 are excluded; request 2 is empty
    idx, score, count = _rank(f, req, 3, 2)
    assert idx == [[5, 2], [7, 4], [-1, -1]] and count == [2, 2, 0]
    assert (score[2] == -INF).all()
    idx, score, count = _rank(f, req, 3, 4)
    assert idx == [[5, 2, -1, -1], [7, 4, 0, -1], [-1, -1, -1, -1]] and count == [2, 3, 0]
    assert (score[0, 2:] == -INF).all() and score[1, 3] == -INF


def test_ref_orderable_is_monotone():
    v = np.array([NAN, -INF, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 0.5, 1.0, 3e38, INF], np.float32)
    o = RR.orderable(v).astype(np.int64)
    assert o[0] == 0 and o[5] == o[6]
    d = np.diff(o)
    assert (np.delete(d, 5) > 0).all()


def test_ref_fuse64():
    p = np.array([[0.5, 0.25], [0.1, 0.9], [0.2, 0.4]], np.float32)
    np.testing.assert_allclose(RR.fuse64(p, [1, 1, 1], 'sum'), p.astype(np.float64).sum(0), rtol=1e-15)
    np.testing.assert_allclose(RR.fuse64(p, [1, 0, 1], 'product'), p[0].astype(np.float64) * p[2], rtol=1e-15)


def test_ref_fma32_rounds_once():
    p = np.random.default_rng(0).random(100, np.float32)
    assert (RR.bits(RR.fma32(np.ones(100, np.float32), p, np.zeros(100, np.float32))) == RR.bits(p)).all()
    # c + a b = (1 + 2^-23) + 2^-24 (1 - 2^-46): just below the f32 tie, so it rounds down; adding in float64 first
    # lands on the tie and would round to even, up
    a, b, c = np.float32(2.0 ** -24 * (1 + 2.0 ** -23)), np.float32(1 - 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    assert float(a) * float(b) == 2.0 ** -24 * (1 - 2.0 ** -46)
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1 + 2.0 ** -22)
    assert RR.fma32([a], [b], [c])[0] == c
    assert RR.fma32([-a], [b], [-c])[0] == -c
    f = RR.fuse32(np.array([[0.5, 0.25], [0.125, 1.0]], np.float32), [2.0, -1.0], 'sum')
    assert f.tolist() == [0.875, -0.5]
    f = RR.fuse32(np.array([[0.5, -0.0], [0.125, 1.0], [0.25, 3.0]], np.float32), [2.0, 0.0, 1.0], 'product')
    assert f.tolist() == [0.125, 0.0] and RR.bits(f)[1] == 0x80000000


# ------------------------------------------------------------------ the library, host side only

@needs_lib
def test_library_exports_rank_symbols():
    lib = _lib.load()
    for s in ('ot_rank_topk', 'ot_rank_topk_workspace_size'):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES and s in _lib.header_symbols()
    txt = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r'int\s+ot_rank_topk\s*\(([^)]*)\)\s*;', txt)
    assert len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib.SIGNATURES['ot_rank_topk'][1]) == 16
    m = re.search(r'size_t\s+ot_rank_topk_workspace_size\s*\(([^)]*)\)\s*;', txt)
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['ot_rank_topk_workspace_size'][1]) == 3
    assert re.search(r'#define\s+OT_RANK_SUM\s+0\b', txt) and re.search(r'#define\s+OT_RANK_PRODUCT\s+1\b', txt)
    assert (_lib.OT_RANK_SUM, _lib.OT_RANK_PRODUCT) == (0, 1)
    assert lib.ot_version() == 20000


@needs_lib
def test_workspace_size_monotone_and_nonzero():
    sz = lambda R, C, K=8: _lib.size('ot_rank_topk_workspace_size', R, C, K)
    assert sz(0, 0) > 0 and sz(1, 1) > 0
    prev = 0
    for C in (0, 1, 255, 256, 1000, 1 << 20, 2 ** 31 - 1):
        cur = sz(4, C)
        assert cur >= prev and cur >= 16 * C
        prev = cur
    prev = 0
    for R in (0, 1, 63, 64, 65, 10000, 1 << 24):
        cur = sz(R, 1000)
        assert cur >= prev and cur >= 8 * R
        prev = cur
    assert sz(1 << 24, 1000) > sz(1, 1000) and sz(4, 1 << 20) > sz(4, 1)


def _call(*, K=4, T=1, C=8, R=2, mode=0, ws_bytes=1 << 20, stride=None):
    """Null pointers throughout: every check below fails before any device work."""
    _lib.call('ot_rank_topk', None, C if stride is None else stride, T, None, mode, None, C, R, K, None, None, None,
              None, None, ws_bytes, None)


@needs_lib
def test_rank_errors_are_reported_not_crashing():
    for K in (0, -1, 1025):
        with pytest.raises(_lib.OneTransHipError, match=r'K=-?\d+ out of range \(1\.\.1024\)'):
            _call(K=K)
    for T in (0, 33):
        with pytest.raises(_lib.OneTransHipError, match=r'1\.\.32 tasks'):
            _call(T=T)
    for C in (2 ** 31, -1):
        with pytest.raises(_lib.OneTransHipError, match='C out of range'):
            _call(C=C, stride=2 ** 32)
    with pytest.raises(_lib.OneTransHipError, match='R=-1 is negative'):
        _call(R=-1)
    with pytest.raises(_lib.OneTransHipError, match='unknown mode 2'):
        _call(mode=2)
    with pytest.raises(_lib.OneTransHipError, match='task_stride < C'):
        _call(stride=7)
    need = _lib.size('ot_rank_topk_workspace_size', 2, 8, 4)
    with pytest.raises(_lib.OneTransHipError, match=f'workspace too small \\({need - 1} < {need}\\)'):
        _call(ws_bytes=need - 1)
    with pytest.raises(_lib.OneTransHipError, match='null operand'):
        _call(ws_bytes=need)
