"""CPU: timestamp-aware sequence fusion — the order's yardstick (tests/time_fusion_ref.py) against hand-written
cases, the config knobs, the host side of ot_seq_time_rows (symbols, header / ctypes agreement, sizing, argument
checks) and the synthetic batches' times."""

import copy
import os
import re

import numpy as np
import pytest

from recommend_amd import _lib
from recommend_amd.config import OneTransConfig, check_seq_fusion, workload_config
from recommend_amd.data import create_sample_batch, criteo_batch, make_batch
from recommend_amd.features import TIME_PAD, SequenceProcessor

import time_fusion_ref as TF

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')
I64_MIN = np.iinfo(np.int64).min


# ------------------------------------------------------------------ the order
def test_ties_go_to_the_earlier_sequence_then_position():
    #      seq 0: 5 5 7     seq 1: 5 6     seq 2: 4 5
    r = TF.merge_ranks([np.array([[5, 5, 7]]), np.array([[5, 6]]), np.array([[4, 5]])])
    # order: s2p0(4) s0p0(5) s0p1(5) s1p0(5) s2p1(5) s1p1(6) s0p2(7)
    assert r.tolist() == [[1, 2, 6, 3, 5, 0, 4]]


def test_unsorted_sequence_still_gives_a_permutation():
    r = TF.merge_ranks([np.array([[9, 3, 3, 1]]), np.array([[2, 8]])])
    assert sorted(r[0].tolist()) == list(range(6))
    # order: s0p3(1) s1p0(2) s0p1(3) s0p2(3) s1p1(8) s0p0(9)
    assert r.tolist() == [[5, 2, 3, 0, 1, 4]]


def test_all_equal_is_the_concatenation():
    r = TF.merge_ranks([np.zeros((2, 3), np.int64), np.zeros((2, 2), np.int64)])
    assert r.tolist() == [[0, 1, 2, 3, 4]] * 2


def test_pads_at_int64_min_sort_first():
    r = TF.merge_ranks([np.array([[I64_MIN, I64_MIN, -5]]), np.array([[I64_MIN, 0]])])
    assert r.tolist() == [[0, 1, 3, 2, 4]]
    assert TIME_PAD == I64_MIN


def test_samples_are_independent():
    a, b = np.array([[3, 1], [1, 3]]), np.array([[2], [2]])
    assert TF.merge_ranks([a, b]).tolist() == [[2, 0, 1], [0, 2, 1]]


# ------------------------------------------------------------------ config
def test_config_defaults_round_trip_and_bad_value():
    cfg = OneTransConfig()
    assert (cfg.seq_fusion, cfg.seq_time_suffix) == ('sep', '_time')
    check_seq_fusion(cfg)
    cfg.seq_fusion, cfg.seq_time_suffix = 'time', '_ts'
    back = OneTransConfig.from_dict(cfg.to_dict())
    assert (back.seq_fusion, back.seq_time_suffix) == ('time', '_ts')
    check_seq_fusion(back)
    old = {k: v for k, v in OneTransConfig().to_dict().items() if k not in ('seq_fusion', 'seq_time_suffix')}
    assert OneTransConfig.from_dict(old).seq_fusion == 'sep'            # a config JSON from before the knob
    cfg.seq_fusion = 'interleave'
    with pytest.raises(ValueError, match='seq_fusion'):
        check_seq_fusion(cfg)


def test_token_count_follows_the_mode():
    cfg = workload_config('C2')
    assert cfg.seq_token_count([42, 42, 42]) == 128
    cfg.seq_fusion = 'time'
    assert cfg.seq_token_count([42, 42, 42]) == 126


# ------------------------------------------------------------------ the library, host side only
@needs_lib
def test_library_exports_seq_time_symbols():
    lib = _lib.load()
    for s in ('ot_seq_time_rows', 'ot_seq_time_rows_workspace_size'):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES and s in _lib.header_symbols()
    txt = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r'int\s+ot_seq_time_rows\s*\(([^)]*)\)\s*;', txt)
    assert len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib.SIGNATURES['ot_seq_time_rows'][1]) == 11
    m = re.search(r'size_t\s+ot_seq_time_rows_workspace_size\s*\(([^)]*)\)\s*;', txt)
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['ot_seq_time_rows_workspace_size'][1]) == 3
    m = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*ot_seq_time\s*;', txt)
    assert [f.split()[-1].lstrip('*') for f in m.group(1).split(';') if f.strip()] == \
        [n for n, _ in _lib.SeqTime._fields_]
    import ctypes
    assert ctypes.sizeof(_lib.SeqTime) == 24
    assert lib.ot_version() == 20000


@needs_lib
def test_workspace_size_monotone():
    sz = lambda B, L, nseq=3: _lib.size('ot_seq_time_rows_workspace_size', B, nseq, L)
    assert sz(0, 1) > 0 and sz(1, 1) > 0
    prev = 0
    for B in (0, 1, 37, 4096, 1 << 20):
        cur = sz(B, 126)
        assert cur >= prev
        prev = cur
    prev = 0
    for L in (1, 2, 63, 64, 65, 126, 1022, 4095, 4096):
        cur = sz(512, L)
        assert cur >= prev > -1
        prev = cur
    assert sz(4, 4097) == 0 and sz(-1, 8) == 0 and sz(4, 8, nseq=0) == 0 and sz(4, 0) == 0


def _call(*, nseq=1, B=2, L_S=4, L=None, stride=None, row_stride=None, ws_bytes=1 << 10, map_off=0):
    """No device pointers (times a dummy non-null address, never read): every check fails before any launch."""
    d = (_lib.SeqTime * 1)(_lib.SeqTime(64, L_S if stride is None else stride, L_S if L is None else L, map_off))
    import ctypes
    _lib.call('ot_seq_time_rows', ctypes.cast(d, ctypes.c_void_p), nseq, B, L_S,
              L_S if row_stride is None else row_stride, None, None, None, None, ws_bytes, None)


@needs_lib
def test_errors_are_reported_before_any_launch():
    E = _lib.OneTransHipError
    for nseq in (0, -1, 33):
        with pytest.raises(E, match=r'nseq=-?\d+ out of range \(1\.\.32\)'):
            _call(nseq=nseq)
    with pytest.raises(E, match='B=-1 is negative'):
        _call(B=-1)
    for L_S in (0, 4097, 1 << 20):
        with pytest.raises(E, match=r'L_S=\d+ unsupported \(1\.\.4096\)'):
            _call(L_S=L_S)
    with pytest.raises(E, match='row_stride < L_S'):
        _call(row_stride=3)
    with pytest.raises(E, match='exceeds int32'):
        _call(B=1 << 20, row_stride=1 << 12)
    need = _lib.size('ot_seq_time_rows_workspace_size', 2, 1, 4)
    with pytest.raises(E, match=f'workspace too small \\({need - 1} < {need}\\)'):
        _call(ws_bytes=need - 1)
    with pytest.raises(E, match='hold 3 events, L_S=4'):
        _call(L=3)
    with pytest.raises(E, match='more than L_S=4'):
        _call(L=5, stride=5)
    with pytest.raises(E, match='stride_b < L'):
        _call(stride=3)
    with pytest.raises(E, match='negative L or map_off'):
        _call(map_off=-1)
    with pytest.raises(E, match='null operand'):
        _call()
    _call(B=0)                                          # an empty batch is a successful no-op


# ------------------------------------------------------------------ host pipeline
def test_pad_times_left_pads_with_int64_min():
    cfg = OneTransConfig()
    cfg.max_seq_len = 4
    sp = SequenceProcessor(cfg)
    out = sp.pad_times([np.array([7, 9]), np.array([], np.int64), np.arange(10, 16)])
    assert out.dtype == np.int64
    assert out.tolist() == [[I64_MIN, I64_MIN, 7, 9], [I64_MIN] * 4, [12, 13, 14, 15]]
    assert sp.process_times([5]).tolist() == [I64_MIN] * 3 + [5]
    assert sp.is_time_key('click_seq_time', {'click_seq': 0}) and not sp.is_time_key('click_seq', {'click_seq': 0})
    assert not sp.is_time_key('other_time', {'click_seq': 0})
    # the event padding is unchanged: zeros
    assert sp.pad_batch([np.ones((1, 64), np.float32)])[0, :3].max() == 0


def _criteo_restated(B, cfg, seed):
    """criteo_batch's NS and sequence draws, restated draw for draw (the generator as it was before times existed)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ns, seq = {}, {}
    for name in cfg.ns_feature_names():
        if name in cfg.sparse_features:
            ns[name] = ((rng.zipf(1.1, size=(B, 1)) - 1) % cfg.sparse_features[name]).astype(np.int64)
        else:
            ns[name] = np.log1p(rng.lognormal(0.0, 1.0, size=(B, 1))).astype(np.float32)
    for name, L in zip(cfg.feature_config['sequence_features'], cfg._seq_lens):
        seq[name] = ((rng.zipf(1.1, size=(B, L)) - 1) % cfg.seq_item_vocab).astype(np.int64)
    return ns, seq


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_sep_batches_are_what_they_were():
    cfg = workload_config('C2')
    cfg._seq_lens = [5, 9, 7]
    ns, seq, lab = make_batch(33, cfg, seed=1234)
    rns, rseq = _criteo_restated(33, cfg, 1234)
    _same(ns, rns)
    _same(seq, rseq)                                    # and no *_time key
    c1 = workload_config('C1')
    ns, seq, _ = make_batch(8, c1, seed=5)
    rng = np.random.Generator(np.random.PCG64(5))
    fc = c1.feature_config
    for name in fc['user_features']:
        assert np.array_equal(ns[name], rng.integers(0, 100, size=(8, 1)).astype(np.float32))
    for name in fc['item_features']:
        assert np.array_equal(ns[name], rng.integers(0, 1000, size=(8, 1)).astype(np.float32))
    for name in fc['context_features']:
        assert np.array_equal(ns[name], rng.random((8, 1), dtype=np.float32))
    assert list(seq) == fc['sequence_features']
    for name, L in zip(fc['sequence_features'], c1._seq_lens):
        assert np.array_equal(seq[name], rng.random((8, L, 64), dtype=np.float32))


@pytest.mark.parametrize('workload', ['C1', 'C2'])
def test_time_batches_add_times_and_change_nothing_else(workload):
    cfg = workload_config(workload)
    cfg._seq_lens = [5, 33, 7]
    sep = make_batch(40, cfg, seed=77)
    tcfg = copy.deepcopy(cfg)
    tcfg.seq_fusion = 'time'
    tim = make_batch(40, tcfg, seed=77)
    names = cfg.feature_config['sequence_features']
    _same(sep[0], tim[0])
    _same(sep[1], {k: tim[1][k] for k in names})
    _same(sep[2], tim[2])
    assert list(tim[1]) == names + [n + '_time' for n in names]
    times = [tim[1][n + '_time'] for n in names]
    for n, t in zip(names, times):
        assert t.dtype == np.int64 and t.shape == tim[1][n].shape[:2]
    again = make_batch(40, tcfg, seed=77)
    _same({k: v for k, v in tim[1].items()}, again[1])                  # seeded
    other = make_batch(40, tcfg, seed=78)
    assert not np.array_equal(other[1][names[1] + '_time'], times[1])
    # the cases the order has to get right are in the data: out-of-order events, ties inside and across sequences
    assert (np.diff(times[1], axis=1) < 0).any()
    assert (np.diff(times[1], axis=1) == 0).any()
    assert np.isin(times[0], times[2]).any()
    r = TF.merge_ranks(times)
    assert (np.sort(r, axis=1) == np.arange(r.shape[1])).all()
    assert (r != np.arange(r.shape[1])).any()                           # really interleaved
    tcfg.seq_time_suffix = '_ts'
    assert names[0] + '_ts' in criteo_batch(4, tcfg, seed=1)[1] if workload == 'C2' else \
        names[0] + '_ts' in create_sample_batch(4, tcfg, seed=1)[1]
