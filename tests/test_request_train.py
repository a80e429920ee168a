"""CPU: request-grouped batches (data.make_request_batch / expand_requests), the float64 cached-attention
reference's own consistency, and the host side of the cached-attention entry points: exported symbols,
header/ctypes agreement and argument validation before any launch."""

import os
import re

import numpy as np
import pytest
import torch

from recommend_amd import _lib
from recommend_amd.config import workload_config
from recommend_amd.data import expand_requests, make_batch, make_request_batch

import request_attn_ref as RA

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')


def _cfg(fusion='sep'):
    cfg = workload_config('C2')
    cfg.hidden_dim, cfg.num_layers, cfg.ffn_dim, cfg.num_ns_tokens = 64, 2, 128, 4
    cfg.sparse_features = {k: 50 for k in cfg.sparse_features}
    cfg.seq_item_vocab = 200
    cfg._seq_lens = [6, 5, 7]
    cfg.seq_fusion = fusion
    return cfg


# ------------------------------------------------------------------ batches

def test_request_batch_shapes_and_req():
    cfg = _cfg()
    ns, seq, labels, req = make_request_batch(5, 3, cfg, seed=11)
    assert req.dtype == np.int32 and req.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3
    assert all(v.shape[0] == 15 for v in ns.values()) and all(v.shape[0] == 15 for v in labels.values())
    assert [v.shape for v in seq.values()] == [(5, 6), (5, 5), (5, 7)]
    assert set(ns) == set(make_batch(15, cfg, seed=11)[0]) and set(labels) == set(cfg.tasks)


def test_request_batch_per_request_list_with_an_empty_request():
    cfg = _cfg()
    ns, seq, labels, req = make_request_batch(4, [3, 0, 4, 1], cfg, seed=5)
    assert req.tolist() == [0, 0, 0, 2, 2, 2, 2, 3] and (np.diff(req) >= 0).all()
    assert all(v.shape[0] == 8 for v in ns.values()) and all(v.shape[0] == 4 for v in seq.values())
    ens, eseq, elab = expand_requests((ns, seq, labels, req))
    assert ens is ns and elab is labels
    for k, v in seq.items():
        assert eseq[k].shape == (8,) + v.shape[1:]
        assert (eseq[k] == v[req]).all()
    with pytest.raises(ValueError):
        make_request_batch(3, [1, 2], cfg)
    with pytest.raises(ValueError):
        make_request_batch(2, [1, -1], cfg)


def test_request_batch_is_deterministic_by_seed():
    cfg = _cfg()
    a, b, c = (make_request_batch(3, [2, 1, 3], cfg, seed=s) for s in (9, 9, 10))
    for x, y in zip(a[:3], b[:3]):
        assert all((x[k] == y[k]).all() for k in x)
    assert (a[3] == b[3]).all()
    assert any((a[1][k] != c[1][k]).any() for k in a[1]) and any((a[0][k] != c[0][k]).any() for k in a[0])


def test_request_batch_carries_times_under_time_fusion():
    cfg = _cfg('time')
    ns, seq, labels, req = make_request_batch(3, [2, 0, 3], cfg, seed=4)
    names = cfg.feature_config['sequence_features']
    times = [n + cfg.seq_time_suffix for n in names]
    assert set(seq) == set(names) | set(times)
    for n, t in zip(names, times):
        assert seq[t].dtype == np.int64 and seq[t].shape == seq[n].shape[:2] and seq[t].shape[0] == 3
    _, eseq, _ = expand_requests((ns, seq, labels, req))
    for t in times:
        assert (eseq[t] == seq[t][req]).all() and eseq[t].shape[0] == 5
    plain = make_request_batch(3, [2, 0, 3], _cfg('sep'), seed=4)
    assert all((plain[1][n] == seq[n]).all() for n in names)       # the other arrays do not depend on the times


# ------------------------------------------------------------------ the reference

def test_reference_sums_a_request_s_candidates():
    g = torch.Generator().manual_seed(3)
    H, hd, Ic, n, Kq, R = 2, 8, 5, 4, 3, 3
    d = H * hd
    req = [0, 0, 0, 2, 2]
    qkv = torch.randn(len(req) * n, 3 * d, generator=g, dtype=torch.float64)
    kv = torch.randn(R * Ic, 2 * d, generator=g, dtype=torch.float64)
    dout = torch.randn(len(req) * Kq, d, generator=g, dtype=torch.float64)
    out, lse, dqkv, dkv = RA.forward_backward(qkv, kv, req, R, H, Ic, n, Kq, dout)
    parts = RA.per_candidate_dkv(qkv, kv, req, R, H, Ic, n, Kq, dout)
    want = torch.zeros(R, Ic, 2 * d, dtype=torch.float64)
    for c, r in enumerate(req):
        want[r] += parts[c]
    torch.testing.assert_close(dkv.reshape(R, Ic, 2 * d), want, rtol=1e-12, atol=1e-12)
    assert (dkv.reshape(R, Ic, 2 * d)[1] == 0).all()                # the request without candidates
    assert (dqkv.reshape(len(req), n, 3 * d)[:, :n - Kq, :d] == 0).all()
    # one candidate against plain causal attention over the concatenated rows
    c = 3
    keys = torch.cat([kv.reshape(R, Ic, 2 * d)[req[c]], qkv.reshape(-1, n, 3 * d)[c][:, d:]], 0)
    q = qkv.reshape(-1, n, 3 * d)[c][n - Kq:, :d]
    for h in range(H):
        s = q[:, h * hd:(h + 1) * hd] @ keys[:, h * hd:(h + 1) * hd].T / np.sqrt(hd)
        mask = torch.arange(Ic + n)[None] <= (Ic + n - Kq + torch.arange(Kq))[:, None]
        s = s.masked_fill(~mask, -1e30)
        o = torch.softmax(s, -1) @ keys[:, d + h * hd:d + (h + 1) * hd]
        torch.testing.assert_close(out.reshape(-1, Kq, d)[c][:, h * hd:(h + 1) * hd], o, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(lse[c, h], torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ the library, host side only

NAMES = ('ot_attn_fwd_cached_lse', 'ot_attn_bwd_cached_workspace_size', 'ot_attn_bwd_cached')


@needs_lib
def test_library_exports_cached_attention_symbols():
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    for s, ret, arity in zip(NAMES, ('int', 'size_t', 'int'), (14, 7, 21)):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES and s in _lib.header_symbols()
        m = re.search(ret + r'\s+' + s + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, s
        assert len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib.SIGNATURES[s][1]) == arity
    # the forward-only export keeps its signature
    m = re.search(r'int\s+ot_attn_fwd_cached\s*\(([^)]*)\)\s*;', txt)
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['ot_attn_fwd_cached'][1]) == 13
    assert lib.ot_version() == 20000


X = 0x1000        # a non-null pointer the library must never follow: every call below fails its checks first


def _fwd(*, qkv=X, ld=24, kv=X, ldc=16, req=X, C=2, H=2, Ic=3, n=4, Kq=2, hd=4, out=X, lse=X):
    _lib.call('ot_attn_fwd_cached_lse', qkv, ld, kv, ldc, req, C, H, Ic, n, Kq, hd, out, lse, None)


def _bwd(*, qkv=X, ld=96, kv=X, ldc=64, rs=X, R=2, C=2, H=2, Ic=3, n=4, Kq=2, hd=16, out=X, dout=X, lse=X, dqkv=X,
         dkv=X, acc=0, ws=X, ws_bytes=1 << 20):
    _lib.call('ot_attn_bwd_cached', qkv, ld, kv, ldc, rs, R, C, H, Ic, n, Kq, hd, out, dout, lse, dqkv, dkv, acc, ws,
              ws_bytes, None)


@needs_lib
def test_cached_forward_lse_rejects_bad_arguments_before_launch():
    for kw in ({'qkv': None}, {'out': None}, {'lse': None}, {'req': None}, {'kv': None}):
        with pytest.raises(_lib.OneTransHipError, match='ot_attn_fwd_cached_lse: null operand'):
            _fwd(**kw)
    with pytest.raises(_lib.OneTransHipError, match='bad sizes'):
        _fwd(Kq=5)                                       # Kq > n
    for kw in ({'n': 0}, {'Kq': 0}, {'C': -1}, {'Ic': -1}, {'H': 0}):
        with pytest.raises(_lib.OneTransHipError, match='bad sizes'):
            _fwd(**kw)
    with pytest.raises(_lib.OneTransHipError, match='ld/ldc'):
        _fwd(ld=20)                                      # ld < 3d
    with pytest.raises(_lib.OneTransHipError, match='ld/ldc'):
        _fwd(ldc=12)                                     # ldc < 2d
    with pytest.raises(_lib.OneTransHipError, match='ld/ldc'):
        _fwd(ld=26)                                      # not a multiple of 4


@needs_lib
def test_cached_backward_rejects_bad_arguments_before_launch():
    for kw in ({'qkv': None}, {'out': None}, {'dout': None}, {'lse': None}, {'dqkv': None}, {'rs': None},
               {'kv': None}, {'dkv': None}, {'ws': None}):
        with pytest.raises(_lib.OneTransHipError, match='ot_attn_bwd_cached: null operand'):
            _bwd(**kw)
    with pytest.raises(_lib.OneTransHipError, match='bad sizes'):
        _bwd(Kq=5)                                       # Kq > n
    for kw in ({'n': 0}, {'Kq': 0}, {'C': -1}, {'R': -1}, {'Ic': -1}, {'H': 0}):
        with pytest.raises(_lib.OneTransHipError, match='bad sizes'):
            _bwd(**kw)
    with pytest.raises(_lib.OneTransHipError, match='head_dim 24 unsupported'):
        _bwd(hd=24, ld=144)
    with pytest.raises(_lib.OneTransHipError, match='ld/ldc'):
        _bwd(ld=92)                                      # ld < 3d
    with pytest.raises(_lib.OneTransHipError, match='ld/ldc'):
        _bwd(ldc=60)                                     # ldc < 2d
    with pytest.raises(_lib.OneTransHipError, match='accumulate'):
        _bwd(acc=2)
    need = _lib.size('ot_attn_bwd_cached_workspace_size', 2, 2, 2, 3, 4, 2, 16)
    assert need >= 2 * 2 * 2 * 2 * 4                     # lse and delta of every (candidate, head, query)
    with pytest.raises(_lib.OneTransHipError, match=f'workspace too small \\({need - 1} < {need}\\)'):
        _bwd(ws_bytes=need - 1)
    assert _lib.size('ot_attn_bwd_cached_workspace_size', 2, 100, 2, 3, 4, 2, 16) > need
    # an empty cache needs no cache pointers
    with pytest.raises(_lib.OneTransHipError, match='workspace too small'):
        _bwd(Ic=0, kv=None, dkv=None, ws_bytes=0)
