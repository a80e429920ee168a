"""CPU: the host side of the weighted, partially labelled multi-task loss and metrics: the ABI of
the new entry points, config validation, ``stack_weights``, the weighted host AUCs, a weighted ``StreamingMetrics``
state finalised on a CPU device, and the two data helpers."""

import os

import numpy as np
import pytest
import torch

from recommend_amd import _lib
from recommend_amd import metrics as M
from recommend_amd.config import OneTransConfig, check_weighted_loss, task_loss_scale, workload_config
from recommend_amd.data import downsample_negatives, gate_task_weights, make_batch, make_request_batch
from recommend_amd.trainer import label_rank, stack_weights

import streaming_metrics_ref as SR
import weighted_ref as WR

NEW = ['ot_task_loss_weighted_workspace_size', 'ot_task_loss_weighted_fwd', 'ot_task_loss_weighted_bwd',
       'ot_metrics_weighted_workspace_size', 'ot_metrics_update_weighted']


def test_header_signatures_and_library_agree():
    hdr = open(_lib.HEADER).read()
    syms = _lib.header_symbols()
    for name in NEW:
        assert name in syms and name in _lib.SIGNATURES, name
    assert '#define OT_METRICS_WEIGHT_ONE (1 << 24)' in hdr
    assert _lib.OT_METRICS_WEIGHT_ONE == 1 << 24 == M.StreamingMetrics.WEIGHT_ONE == WR.UNIT
    assert _lib.OT_LOSS_WEIGHT_MAX == 65536 and _lib.LOSS_REDUCTIONS == {'batch': 0, 'weights': 1}
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libonetrans_hip.so is not built')
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ot_version() == 20000
    # host-only size queries: {sum w l, sum w} doubles per (task, workgroup), at most 256 workgroups per task;
    # 3 doubles and one 64-bit integer per (task, workgroup), at most 128
    assert lib.ot_task_loss_weighted_workspace_size(3, 257) == 3 * 2 * 2 * 8
    assert lib.ot_task_loss_weighted_workspace_size(3, 1 << 20) == 3 * 256 * 2 * 8
    assert lib.ot_metrics_weighted_workspace_size(3, 1027) == 3 * 2 * 32
    assert lib.ot_metrics_weighted_workspace_size(3, 1 << 20) == 3 * 128 * 32


def test_bad_arguments_are_refused_without_device_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libonetrans_hip.so is not built')
    fwd = lambda *a: _lib.call('ot_task_loss_weighted_fwd', *a)
    p = 4096                                                    # a non-null, aligned dummy address: never read
    with pytest.raises(_lib.OneTransHipError, match='null operand'):
        fwd(None, p, p, None, 0, None, 2, 8, 0, 0, p, p, p, 1 << 20, None)
    with pytest.raises(_lib.OneTransHipError, match='1..32 tasks'):
        fwd(None, p, p, p, 0, None, 33, 8, 0, 0, p, p, p, 1 << 20, None)
    with pytest.raises(_lib.OneTransHipError, match='empty batch'):
        fwd(None, p, p, p, 0, None, 2, 0, 0, 0, p, p, p, 1 << 20, None)
    with pytest.raises(_lib.OneTransHipError, match='unknown reduction'):
        fwd(None, p, p, p, 0, None, 2, 8, 0, 2, p, p, p, 1 << 20, None)
    with pytest.raises(_lib.OneTransHipError, match='weight_stride'):
        fwd(None, p, p, p, 7, None, 2, 8, 0, 0, p, p, p, 1 << 20, None)
    with pytest.raises(_lib.OneTransHipError, match='workspace'):
        fwd(None, p, p, p, 0, None, 2, 8, 0, 0, p, p, p, 8, None)
    with pytest.raises(_lib.OneTransHipError, match='null operand'):
        _lib.call('ot_task_loss_weighted_bwd', p, p, p, 0, None, None, p, 2, 8, 0, 0, p, None)
    with pytest.raises(_lib.OneTransHipError, match='null operand'):
        _lib.call('ot_metrics_update_weighted', p, p, None, 2, 8, 8, 0, p, 4, p, p, p, 1 << 20, None)
    with pytest.raises(_lib.OneTransHipError, match='weight_stride'):
        _lib.call('ot_metrics_update_weighted', p, p, p, 2, 8, 8, 4, p, 4, p, p, p, 1 << 20, None)


def test_config_validation():
    cfg = workload_config('C2')
    assert cfg.weighted_loss is False and cfg.loss_reduction == 'batch' and cfg.task_loss_weights == {}
    assert cfg.sample_weight_key == 'sample_weight' and cfg.label_weight_suffix == '_weight'
    check_weighted_loss(cfg)
    assert task_loss_scale(cfg) is None
    cfg.weighted_loss, cfg.loss_reduction, cfg.task_loss_weights = True, 'weights', {'cvr': 0.25, 'ctr': 0}
    check_weighted_loss(cfg)
    assert task_loss_scale(cfg) == [0.0, 0.25]
    back = OneTransConfig.from_dict(cfg.to_dict())
    assert back.weighted_loss is True and back.loss_reduction == 'weights' and back.task_loss_weights == {'cvr': 0.25, 'ctr': 0}
    for attr, bad in [('loss_reduction', 'mean'), ('loss_reduction', None), ('task_loss_weights', {'cvr': -1.0}),
                      ('task_loss_weights', {'cvr': float('nan')}), ('task_loss_weights', {'cvr': float('inf')}),
                      ('task_loss_weights', {'cvr': '1'}), ('task_loss_weights', {'ctcvr': 1.0}),
                      ('sample_weight_key', ''), ('label_weight_suffix', ''), ('sample_weight_key', 'ctr')]:
        c = OneTransConfig.from_dict(cfg.to_dict())
        setattr(c, attr, bad)
        with pytest.raises(ValueError):
            check_weighted_loss(c)


def test_stack_weights_shapes_and_missing_keys():
    cfg = workload_config('C2')                                  # tasks ctr, cvr
    B = 6
    lab = {'ctr': np.zeros((B, 1), np.float32), 'cvr': np.full((B, 1), np.nan, np.float32)}
    assert stack_weights(lab, cfg, 'cpu') is None
    assert stack_weights(torch.zeros(2, B), cfg, 'cpu') is None
    sw = np.arange(B, dtype=np.float32)
    cw = np.array([1, 0, 1, 0, 2, 0.5], np.float64).reshape(B, 1)
    w = stack_weights(dict(lab, sample_weight=sw), cfg, 'cpu')
    assert w.shape == (2, B) and w.dtype == torch.float32 and w.stride(0) == 0
    assert torch.equal(w[0], torch.from_numpy(sw)) and torch.equal(w[1], w[0])
    w = stack_weights(dict(lab, cvr_weight=cw), cfg, 'cpu')
    assert torch.equal(w, torch.stack([torch.ones(B), torch.from_numpy(cw.reshape(-1)).float()]))
    w = stack_weights(dict(lab, sample_weight=sw.reshape(B, 1), cvr_weight=torch.from_numpy(cw)), cfg, 'cpu')
    assert torch.equal(w, torch.stack([torch.from_numpy(sw), torch.from_numpy(sw * cw.reshape(-1).astype(np.float32))]))
    cfg.sample_weight_key, cfg.label_weight_suffix = 'w', '__w'  # the names come from the config
    assert stack_weights(dict(lab, sample_weight=sw), cfg, 'cpu') is None
    assert torch.equal(stack_weights(dict(lab, ctr__w=sw), cfg, 'cpu')[0], torch.from_numpy(sw))
    # the extra keys do not change which BCE form the labels select
    assert label_rank(dict({'ctr': np.zeros(B), 'cvr': np.zeros(B)}, sample_weight=sw.reshape(B, 1)),
                      cfg.tasks) == 1


@pytest.mark.parametrize('bad', [np.nan, -0.5, 65537.0, np.inf])
def test_stack_weights_refuses_bad_host_values(bad):
    cfg = workload_config('C2')
    B = 5
    lab = {'ctr': np.zeros((B, 1), np.float32), 'cvr': np.zeros((B, 1), np.float32)}
    for key in ('sample_weight', 'cvr_weight'):
        w = np.ones(B, np.float32)
        w[3] = bad
        with pytest.raises(ValueError, match='weights must lie in'):
            stack_weights(dict(lab, **{key: w}), cfg, 'cpu')
    ok = np.array([0.0, 65536.0, 1.0, 2.5, 1e-30], np.float32)    # both ends of the range are legal
    assert stack_weights(dict(lab, sample_weight=ok), cfg, 'cpu') is not None


def test_stack_weights_refuses_wrong_length_shape_and_dtype():
    cfg = workload_config('C2')
    B = 5
    lab = {'ctr': np.zeros((B, 1), np.float32), 'cvr': np.zeros((B, 1), np.float32)}
    for w in (np.ones(B + 1, np.float32), np.ones((B, 2), np.float32), np.ones((1, B), np.float32),
              np.ones((B, 1, 1), np.float32)):
        with pytest.raises(ValueError, match='shape'):
            stack_weights(dict(lab, sample_weight=w), cfg, 'cpu')
    with pytest.raises(ValueError, match='floating-point'):
        stack_weights(dict(lab, sample_weight=np.ones(B, np.int64)), cfg, 'cpu')


def test_weighted_auc_equals_replicated_records():
    rng = np.random.default_rng(5)
    n = 300
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = np.round(rng.random(n), 2).astype(np.float32)            # many ties
    k = rng.integers(0, 5, n)                                    # zeros drop records
    yr, sr = np.repeat(y, k), np.repeat(s, k)
    assert M.auc(y, s, weights=k) == M.auc(yr, sr)
    assert M.auc(y, s, weights=np.ones(n)) == M.auc(y, s)
    assert M.keras_auc(y, s, weights=k) == pytest.approx(M.keras_auc(yr, sr), rel=1e-13)
    assert M.keras_auc(y, s, weights=np.ones(n)) == pytest.approx(M.keras_auc(y, s), rel=1e-13)
    # zero-weight records may hold anything
    y2, s2, k2 = np.append(y, np.nan), np.append(s, np.nan), np.append(k, 0)
    assert M.auc(y2, s2, weights=k2) == M.auc(yr, sr)
    assert M.keras_auc(y2, s2, weights=k2) == M.keras_auc(y, s, weights=k)
    # fractional weights: the pair statistic
    w = rng.random(n)
    pos, neg = y > 0.5, y <= 0.5
    gt = (s[pos][:, None] > s[neg][None, :]) + 0.5 * (s[pos][:, None] == s[neg][None, :])
    want = float((w[pos][:, None] * w[neg][None, :] * gt).sum() / (w[pos].sum() * w[neg].sum()))
    assert M.auc(y, s, weights=w) == pytest.approx(want, rel=1e-12)
    assert np.isnan(M.auc(y, s, weights=np.where(pos, 1.0, 0.0)))          # a class without weight
    with pytest.raises(ValueError):
        M.auc(y, s, weights=np.ones(n - 1))
    with pytest.raises(ValueError):
        M.auc(y, s, weights=-np.ones(n))


def test_weighted_streaming_state_finalised_on_cpu():
    """A hand-built weighted state (the numpy reference's) loaded into a CPU object: ``result`` equals Keras's
    weighted metrics straight from the samples."""
    tasks, B = ['ctr', 'cvr', 'watch'], 500
    y, p = SR.make_inputs(3, B, seed=3)
    y[1] = (y[1] > 0.5).astype(np.float32)
    rng = np.random.default_rng(4)
    w = rng.choice([0.0, 0.25, 1.0, 3.0, 1.0 / 0.3], size=(3, B)).astype(np.float32)
    y[1][w[1] == 0] = np.nan                                     # a zero weight hides a missing label
    m = M.StreamingMetrics(tasks, 'cpu', weighted=True)
    assert m.weighted and not M.StreamingMetrics(tasks, 'cpu').weighted
    counts, sums = WR.ref_state_weighted(y, p, w, m.bounds_host)
    m.load_state(counts, sums)
    res = m.result(extended=True)
    for i, t in enumerate(tasks):
        want = WR.weighted_metrics(y[i], p[i], w[i], m.thresholds, binary=t != 'watch')
        for k, v in want.items():
            assert np.isfinite(v)
            assert res[f'{t}_{k}'] == pytest.approx(v, rel=1e-12, abs=1e-15), (t, k)
    # an all-zero task reports zeros (div_no_nan), not NaN
    counts[1], sums[1] = 0, 0
    m.load_state(counts, sums)
    res = m.result(extended=True)
    assert all(res[f'cvr_{k}'] == 0.0 for k in ('auc', 'accuracy', 'precision', 'recall', 'f1', 'logloss'))
    with pytest.raises(ValueError, match='weighted=True'):
        M.StreamingMetrics(tasks, 'cpu').update(torch.zeros(3, 4), torch.zeros(3, 4), weights=torch.ones(4))


def test_gate_task_weights():
    cfg = workload_config('C2')
    _, _, lab = make_batch(40, cfg, seed=1000, seq_lens=[4, 4, 4])
    out = gate_task_weights(lab)
    assert set(out) == set(lab) | {'cvr_weight'} and 'cvr_weight' not in lab
    assert out['cvr_weight'].dtype == np.float32 and out['cvr_weight'].shape == lab['ctr'].shape
    assert np.array_equal(out['cvr_weight'], (lab['ctr'] > 0.5).astype(np.float32))
    assert 0 < out['cvr_weight'].sum() < 40
    assert 'ctr__w' in gate_task_weights(lab, task='ctr', gate='cvr', suffix='__w')
    with pytest.raises(KeyError):
        gate_task_weights(lab, task='ctcvr')


def test_downsample_negatives():
    cfg = workload_config('C2')
    B = 400
    ns, seq, lab = make_batch(B, cfg, seed=1000, seq_lens=[4, 4, 4])
    ns = dict(ns, row_index=np.arange(B, dtype=np.int64).reshape(B, 1))      # tells which rows were kept
    batch = (ns, seq, lab)
    ns2, seq2, lab2 = downsample_negatives(batch, 'ctr', 0.25, seed=3)
    y = lab['ctr'].reshape(-1)
    rows = ns2['row_index'].reshape(-1)
    n = len(rows)
    assert np.all(np.diff(rows) > 0)                                         # rows of the batch, in order
    assert set(np.nonzero(y > 0.5)[0]) <= set(rows)                          # every positive is kept
    kept_neg = int((y[rows] <= 0.5).sum())
    assert 0 < kept_neg < int((y <= 0.5).sum()) and abs(kept_neg - 0.25 * (y <= 0.5).sum()) < 40
    for d, d2 in ((ns, ns2), (seq, seq2), (lab, lab2)):                      # every array cut alike
        assert set(d2) - {'sample_weight'} == set(d)
        assert all(np.array_equal(d2[k], d[k][rows]) for k in d)
    w2 = lab2['sample_weight']
    assert w2.dtype == np.float32 and w2.shape == lab2['ctr'].shape
    assert np.array_equal(w2.reshape(-1), np.where(y[rows] > 0.5, np.float32(1.0), np.float32(4.0)))
    key = 'row_index'
    again = downsample_negatives(batch, 'ctr', 0.25, seed=3)
    assert all(np.array_equal(again[2][k], lab2[k]) for k in lab2)           # same seed, same cut
    other = downsample_negatives(batch, 'ctr', 0.25, seed=4)
    assert len(other[2]['ctr']) != n or not np.array_equal(other[0][key], ns2[key])
    # an existing sample weight is multiplied in; keep_rate 1 keeps everything
    lab_w = dict(lab, sample_weight=np.full((B, 1), 2.0, np.float32))
    full = downsample_negatives((ns, seq, lab_w), 'ctr', 1.0, seed=0)
    assert len(full[2]['ctr']) == B and np.all(full[2]['sample_weight'] == 2.0)
    # request-grouped: the candidate side is cut, the request side stays
    rb = make_request_batch(3, [5, 0, 6], cfg, seed=1000, seq_lens=[4, 4, 4])
    ns4, seq4, lab4, req4 = downsample_negatives(rb, 'ctr', 0.5, seed=1)
    assert len(req4) == len(lab4['ctr']) == len(next(iter(ns4.values()))) <= 11
    assert all(np.array_equal(seq4[k], rb[1][k]) for k in rb[1]) and np.all(np.diff(req4) >= 0)
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError):
            downsample_negatives(batch, 'ctr', bad, seed=0)
