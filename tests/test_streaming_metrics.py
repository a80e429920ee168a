"""CPU: ``StreamingMetrics`` finalises a metric state into the reference's numbers (against oracle.keras_math and
closed forms — never against itself), merges states over ranks, and ``OneTransTrainer.fit`` runs the
reference's epoch loop (train.py:192-279).  The kernel that builds the state is checked on the GPU
(test_streaming_metrics_gpu.py); here the state comes from the float64 numpy restatement."""

import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.keras_math import auc_keras, keras_bce
from recommend_amd import _lib
from recommend_amd.metrics import StreamingMetrics
from recommend_amd.trainer import OneTransTrainer

import streaming_metrics_ref as R

TASKS = ['ctr', 'cvr', 'watch_time']
BINARY_KEYS = ('auc', 'accuracy', 'precision', 'recall', 'f1', 'logloss')


def loaded(y, p, tasks=TASKS):
    m = StreamingMetrics(tasks, 'cpu')
    assert np.array_equal(m.bounds_host, R.bounds()) and m.nb == 201
    m.load_state(*R.ref_state(y, p))
    return m


def test_result_matches_keras_and_closed_forms():
    y, p = R.make_inputs(3, 1000, seed=11)
    y[1] = (y[1] > 0.3).astype(np.float32)
    for v in R.special_probs():                         # the edges of every bin are among the samples
        assert np.any(p[0] == v)
    res = loaded(y, p).result(extended=True)
    assert set(res) == {f'{t}_{k}' for t in ('ctr', 'cvr') for k in BINARY_KEYS} | {'watch_time_mse', 'watch_time_mae'}
    assert set(loaded(y, p).result()) == ({f'{t}_{k}' for t in ('ctr', 'cvr') for k in BINARY_KEYS[:4]}
                                          | {'watch_time_mse', 'watch_time_mae'})
    for i, t in enumerate(('ctr', 'cvr')):
        cf = R.closed_forms(y[i], p[i])
        assert abs(res[f'{t}_auc'] - auc_keras(y[i], p[i])) < 1e-12
        for k in ('accuracy', 'precision', 'recall', 'f1'):
            assert abs(res[f'{t}_{k}'] - cf[k]) < 1e-12, (t, k)
        assert abs(res[f'{t}_logloss'] - keras_bce(y[i].astype(np.float64), p[i].astype(np.float64))) < 1e-12
    cf = R.closed_forms(y[2], p[2])
    assert abs(res['watch_time_mse'] - cf['mse']) < 1e-12
    assert abs(res['watch_time_mae'] - cf['mae']) < 1e-12


@pytest.mark.parametrize('case', ['all_negative', 'all_positive', 'none_above_half', 'empty'])
def test_degenerate_states_report_zero_not_nan(case):
    y, p = R.make_inputs(2, 300, seed=5)
    y[1] = y[0]
    if case == 'all_negative':
        y[:] = 0.0
    elif case == 'all_positive':
        y[:] = 1.0
    elif case == 'none_above_half':
        p = np.minimum(p, np.float32(0.5))
    p[1] = p[0]                                         # both tasks see the same samples
    m = loaded(y, p, ['ctr', 'cvr'])
    if case == 'empty':
        m.reset_states()
    res = m.result(extended=True)
    assert all(math.isfinite(v) for v in res.values()), res
    zero = {'all_negative': ('auc', 'precision', 'recall', 'f1'),     # no positives: TP = 0, recall's denominator 0
            'all_positive': ('auc',),                                 # no negatives: the false-positive rate is 0/0
            'none_above_half': ('precision', 'recall', 'f1'),         # nothing predicted positive
            'empty': BINARY_KEYS}[case]
    for t in ('ctr', 'cvr'):
        for k in zero:
            assert res[f'{t}_{k}'] == 0.0, (t, k)
        if case != 'empty':
            cf = R.closed_forms(y[0], p[0])
            for k in ('accuracy', 'precision', 'recall', 'f1'):
                assert abs(res[f'{t}_{k}'] - cf[k]) < 1e-12
            assert abs(res[f'{t}_auc'] - auc_keras(y[0], p[0])) < 1e-12


# ---------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        y, p = R.make_inputs(3, 600, seed=21)
        sl = slice(300 * rank, 300 * rank + 300)
        m = StreamingMetrics(TASKS, 'cpu')
        m.load_state(*R.ref_state(y[:, sl], p[:, sl]))
        m.all_reduce()
        q.put((rank, m.result(extended=True), m.state()[0].numpy().copy(), m.state()[1].numpy().copy()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_merges_the_ranks_states():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for pr in procs:
        pr.join(120)
        assert pr.exitcode == 0
    y, p = R.make_inputs(3, 600, seed=21)
    (ca, sa), (cb, sb) = R.ref_state(y[:, :300], p[:, :300]), R.ref_state(y[:, 300:], p[:, 300:])
    whole = StreamingMetrics(TASKS, 'cpu')              # one process that saw both halves
    whole.load_state(ca + cb, sa + sb)
    want = whole.result(extended=True)
    assert sorted(g[0] for g in got) == [0, 1]
    for _, res, counts, sums in got:
        assert res == want
        assert np.array_equal(counts, R.ref_state(y, p)[0])
        assert np.array_equal(sums, sa + sb)
    assert abs(want['ctr_auc'] - auc_keras(y[0], p[0])) < 1e-12


# ---------------------------------------------------------------- fit(): the reference's control flow
class _Cfg:
    tasks = ['ctr']


class ScriptedTrainer(OneTransTrainer):
    """fit() over stub steps: validation losses from a script, checkpoints recorded instead of written."""

    def __init__(self, val_losses):
        self.config = _Cfg()
        self.device = torch.device('cpu')
        self.history = {'train_loss': [], 'val_loss': [], 'train_metrics': {}, 'val_metrics': {}}
        self.train_metrics = self.val_metrics = None
        self.val_losses = list(val_losses)
        self.epoch = 0
        self.saved = []
        self.state_at_epoch_start = []

    def train_step(self, batch_data, next_batch=None):
        counts, sums = self.train_metrics.state()
        if batch_data == 0:
            self.epoch += 1
            self.state_at_epoch_start.append((int(counts.sum()), float(sums.sum()),
                                              int(self.val_metrics.state()[0].sum())))
        counts[0, 1, -1] += 1                            # a positive sample above every threshold
        sums[0, 0] += 1.0
        return {'total_loss': torch.tensor(2.0)}

    def val_step(self, batch_data):
        self.val_metrics.state()[0][0, 0, 0] += 1
        return {'total_loss': torch.tensor(self.val_losses[self.epoch - 1])}

    def save_model(self, model_name):
        self.saved.append((self.epoch, model_name))


def test_fit_control_flow():
    tr = ScriptedTrainer([1.0, 0.9, 0.95, 0.97, 0.5])
    hist = tr.fit([0, 1, 2], [0], epochs=5, save_freq=2, early_stopping_patience=2)
    assert tr.epoch == 4                                 # two epochs without improvement after epoch 2
    assert tr.saved == [(1, 'best_model'), (2, 'best_model'), (2, 'model_epoch_2'), (4, 'model_epoch_4'),
                        (4, 'final_model')]
    assert [round(v, 6) for v in hist['val_loss']] == [1.0, 0.9, 0.95, 0.97]
    assert hist['train_loss'] == [2.0] * 4
    assert tr.state_at_epoch_start == [(0, 0.0, 0)] * 4  # both states reset between epochs
    assert sorted(hist['train_metrics']) == sorted(hist['val_metrics']) == [0, 1, 2, 3]
    for ep in range(4):
        assert set(hist['train_metrics'][ep]) == {'ctr_auc', 'ctr_accuracy', 'ctr_precision', 'ctr_recall'}
        assert hist['train_metrics'][ep]['ctr_recall'] == 1.0       # three positives, all predicted positive
        assert hist['val_metrics'][ep]['ctr_accuracy'] == 1.0       # one negative below 0.5


def test_fit_without_validation_uses_the_train_loss():
    tr = ScriptedTrainer([])
    hist = tr.fit([0, 1], None, epochs=2, save_freq=5, early_stopping_patience=5)
    assert hist['val_loss'] == hist['train_loss'] == [2.0, 2.0]
    assert tr.saved == [(1, 'best_model'), (2, 'final_model')]


# ---------------------------------------------------------------- the C ABI's argument checks (host only)
@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')
def test_metrics_update_argument_errors():
    """Every argument error returns OT_ERR_INVALID_ARG with a message before any device work (the pointers
    below are never dereferenced)."""
    T, B, nb = 2, 64, 201
    ws = _lib.size('ot_metrics_workspace_size', T, B)
    assert ws >= T * 3 * 8                               # answered on the host: a partial per task at least
    assert _lib.size('ot_metrics_workspace_size', 32, 1 << 20) >= ws
    a = 4096                                             # a non-null, aligned stand-in for every pointer
    good = dict(probs=a, labels=a, T=T, B=B, stride=B, bounds=a, nb=nb, counts=a, sums=a, ws=a, ws_bytes=ws)

    def call(**kw):
        g = dict(good, **kw)
        _lib.call('ot_metrics_update', g['probs'], g['labels'], g['T'], g['B'], g['stride'], g['bounds'], g['nb'],
                  g['counts'], g['sums'], g['ws'], g['ws_bytes'], None)

    for name in ('probs', 'labels', 'bounds', 'counts', 'sums', 'ws'):
        with pytest.raises(_lib.OneTransHipError, match='null operand'):
            call(**{name: None})
    for T_bad in (0, 33):
        with pytest.raises(_lib.OneTransHipError, match='tasks'):
            call(T=T_bad)
    for nb_bad in (0, 1025):
        with pytest.raises(_lib.OneTransHipError, match='thresholds'):
            call(nb=nb_bad)
    with pytest.raises(_lib.OneTransHipError, match='empty batch'):
        call(B=0, stride=0)
    with pytest.raises(_lib.OneTransHipError, match='task_stride'):
        call(stride=B - 1)
    with pytest.raises(_lib.OneTransHipError, match='workspace too small'):
        call(ws_bytes=ws - 1)
    assert _lib.load().ot_version() == 20000
