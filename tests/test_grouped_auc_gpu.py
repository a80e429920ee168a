"""GPU: ``ot_grouped_auc`` against the pair-counting yardstick (grouped_auc_ref) — the per-group integers and the
distinct ids exactly, the double sums within the summation order — its bit-reproducibility, also under a permutation
of the records; ``GroupedAUC``'s log; and the trainer's / evaluator's ``{t}_uauc`` on the probabilities the model
produced."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd.data import make_batch
from recommend_amd.evaluate import OneTransEvaluator
from recommend_amd.metrics import GroupedAUC, uauc
from recommend_amd.model import OneTransModel
from recommend_amd.trainer import OneTransTrainer

import grouped_auc_ref as R
from test_model_gpu import small_criteo

# agg[:, 0:2]: only the summation order differs from the yardstick (G * 2^-53 < 1.2e-12 for G <= 10^4 groups)
SUM_RTOL = 1e-12


def run_kernel(g, y, s, bits, binary, dev, labels=None, scores=None, stride=None):
    """One ot_grouped_auc call -> (agg [T, 4], ids [G], stats [T, G, 3]) on the host.  ``labels`` / ``scores``:
    device tensors to use in place of ``y`` / ``s`` (rows ``stride`` apart)."""
    T, n = y.shape
    gd = torch.from_numpy(np.array(g, order='C')).to(dev)
    yd = labels if labels is not None else torch.from_numpy(np.array(y, order='C')).to(dev)
    sd = scores if scores is not None else torch.from_numpy(np.array(s, order='C')).to(dev)
    assert yd.stride(1) == 1 and sd.stride(1) == 1 and yd.stride(0) == sd.stride(0) == (stride or n)
    agg = torch.full((T, 4), -1.0, dtype=torch.float64, device=dev)
    num = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ids = torch.full((n,), -1, dtype=torch.int64, device=dev)
    stats = torch.full((T, n, 3), -1, dtype=torch.int64, device=dev)
    mask = sum(1 << t for t, b in enumerate(binary) if b)
    K.grouped_auc(gd, sd, yd, T, n, stride or n, bits, mask, agg, num, ids, stats, device=dev)
    G = int(num.item())
    assert not stats[:, G:].any()                        # rows past the distinct groups are zero
    return agg.cpu().numpy(), ids[:G].cpu().numpy(), stats[:, :G].cpu().numpy()


@pytest.mark.parametrize('name', list(R.CASES))
def test_kernel_matches_the_yardstick(dev, name):
    g, y, s, bits, binary, refs = R.case(name)
    agg, ids, stats = run_kernel(g, y, s, bits, binary, dev)
    for t, ref in enumerate(refs):
        if ref is None:                                  # masked off: zeros
            assert not agg[t].any() and not stats[t].any()
            continue
        assert np.array_equal(ids, ref['ids'])
        assert np.array_equal(stats[t], ref['stats'])
        assert np.array_equal(agg[t, 2:], ref['agg'][2:])
        assert R.rel_close(agg[t, :2], ref['agg'][:2], SUM_RTOL), (agg[t], ref['agg'])


def test_no_outputs_beyond_agg_are_required(dev):
    g, y, s, bits, binary, refs = R.case('ties')
    T, n = y.shape
    agg = torch.empty((T, 4), dtype=torch.float64, device=dev)
    num = torch.empty((1,), dtype=torch.int64, device=dev)
    K.grouped_auc(torch.from_numpy(np.array(g)).to(dev), torch.from_numpy(np.array(s)).to(dev),
                  torch.from_numpy(np.array(y)).to(dev), T, n, n, bits, 3, agg, num, device=dev)
    assert int(num.item()) == len(refs[0]['ids'])
    assert agg.cpu().numpy().tobytes() == run_kernel(g, y, s, bits, binary, dev)[0].tobytes()


@pytest.mark.parametrize('name', ['ties', 'zipf_crawler', 'wide_ids_masked'])
def test_result_is_bit_reproducible_also_under_a_permutation(dev, name):
    g, y, s, bits, binary, _ = R.case(name)
    a = run_kernel(g, y, s, bits, binary, dev)
    b = run_kernel(g, y, s, bits, binary, dev)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])
    perm = np.random.default_rng(3).permutation(len(g))
    c = run_kernel(g[perm], y[:, perm], s[:, perm], bits, binary, dev)
    assert a[0].tobytes() == c[0].tobytes()
    assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])


def test_strided_misaligned_rows_equal_packed(dev):
    """task_stride > n and base pointers one float off a 16-byte boundary."""
    g, y, s, bits, binary, _ = R.case('ties')
    T, n, stride = 2, 257, 301
    packed = run_kernel(g, y, s, bits, binary, dev)
    bufs = []
    for a in (y, s):
        buf = torch.full((T * stride + 1,), 0.75, dtype=torch.float32, device=dev)     # the padding is not read
        v = buf[1:].view(T, stride)[:, :n]
        v.copy_(torch.from_numpy(np.array(a)))
        assert v.data_ptr() % 16 == 4 and v.stride(0) == stride
        bufs.append(v)
    got = run_kernel(g, y, s, bits, binary, dev, labels=bufs[0], scores=bufs[1], stride=stride)
    assert got[0].tobytes() == packed[0].tobytes()
    assert np.array_equal(got[1], packed[1]) and np.array_equal(got[2], packed[2])


# ---------------------------------------------------------------- GroupedAUC
TASKS = ['ctr', 'cvr']


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def test_updates_accumulate_grow_and_reset(dev):
    g, y, s, bits, _, refs = R.case('zipf_crawler')
    perm = np.random.default_rng(5).permutation(4096)
    parts = [np.arange(100), np.arange(100, 101), perm]  # updates of B = 100, 1 and 4096
    m = GroupedAUC(TASKS, dev, capacity=64)              # grows from 64
    for k, i in enumerate(parts):
        ids = _dev(g[i], dev)
        m.update(ids.reshape(-1, 1) if k == 0 else ids, _dev(y[:, i], dev), _dev(s[:, i], dev))
    assert m.count == 4197 and m.capacity >= 4197
    idx = np.concatenate(parts)
    G2, Y2, S2 = g[idx], y[:, idx], s[:, idx]
    one = GroupedAUC(TASKS, dev)
    one.update(_dev(G2, dev), _dev(Y2, dev), _dev(S2, dev))
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(m.state(), one.state()))
    got, want = m.result(per_group=True), one.result(per_group=True)
    _same(got, want)
    for i, t in enumerate(TASKS):
        ref = R.ref_uauc(G2, Y2[i], S2[i])
        assert np.array_equal(got['groups'], ref['ids']) and np.array_equal(got[f'{t}_group_stats'], ref['stats'])
        assert R.rel_close(got[f'{t}_uauc'], ref['uauc'], SUM_RTOL)
        assert got[f'{t}_uauc_users'] == ref['users'] and got[f'{t}_uauc_impressions'] == ref['impressions']
    m.reset_states()
    assert m.count == 0 and m.result() == {f'{t}_{k}': 0 for t in TASKS
                                           for k in ('uauc', 'uauc_macro', 'uauc_users', 'uauc_impressions')}
    m.update(_dev(g[:63], dev), _dev(y[:, :63], dev), _dev(s[:, :63], dev))              # and it fills again
    assert m.result()['ctr_uauc_impressions'] == R.ref_uauc(g[:63], y[0, :63], s[0, :63])['impressions']


def test_result_per_group_matches_the_yardstick(dev):
    g, y, s, bits, binary, refs = R.case('wide_ids_masked')
    m = GroupedAUC(['ctr', 'cvr', 'watch_time'], dev, capacity=1 << 14)
    m.update(_dev(g, dev), _dev(y, dev), _dev(s, dev))
    res = m.result(per_group=True)
    assert not any(k.startswith('watch_time') for k in res)
    assert np.array_equal(res['groups'], refs[0]['ids'])
    for i, t in enumerate(['ctr', 'cvr']):
        assert np.array_equal(res[f'{t}_group_stats'], refs[i]['stats'])
        assert R.rel_close(res[f'{t}_uauc'], refs[i]['uauc'], SUM_RTOL)
        assert R.rel_close(res[f'{t}_uauc_macro'], refs[i]['uauc_macro'], SUM_RTOL)
        assert res[f'{t}_uauc_users'] == refs[i]['users'] and res[f'{t}_uauc_impressions'] == refs[i]['impressions']
    assert set(m.result()) == {f'{t}_{k}' for t in ('ctr', 'cvr')
                               for k in ('uauc', 'uauc_macro', 'uauc_users', 'uauc_impressions')}


def test_update_checks_its_arguments(dev):
    m = GroupedAUC(TASKS, dev, capacity=8)
    g, y = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(2, 4, device=dev)
    with pytest.raises(ValueError):
        m.update(g, y, y[:1])
    with pytest.raises(ValueError):
        m.update(g.to(torch.int32), y, y)
    with pytest.raises(ValueError):
        m.update(g[:3], y, y)
    with pytest.raises(K._lib.OneTransHipError, match='GPU only'):
        m.update(g.cpu(), y.cpu(), y.cpu())
    assert m.count == 0


# ---------------------------------------------------------------- trainer / evaluator
FEATURE = 'C1'      # a sparse id feature of the Criteo-shape batch: 40 distinct values, Zipf-distributed


def _batches(cfg, n, seed=300):
    return [make_batch(24, cfg, seed=seed + i) for i in range(n)]


def _records(batches, probs, tasks):
    G = np.concatenate([np.asarray(b[0][FEATURE]).reshape(-1) for b in batches]).astype(np.int64)
    Y = np.stack([np.concatenate([np.asarray(b[2][t], dtype=np.float32).reshape(-1) for b in batches]) for t in tasks])
    return G, Y, np.concatenate(probs, 1)


UAUC_KEYS = ('uauc', 'uauc_macro', 'uauc_users', 'uauc_impressions')


def _check_against_host(res, G, Y, P, tasks):
    for i, t in enumerate(tasks):
        host = uauc(G, Y[i], P[i])
        assert host['users'] > 0
        assert R.rel_close(res[f'{t}_uauc'], host['uauc'], SUM_RTOL)
        assert R.rel_close(res[f'{t}_uauc_macro'], host['uauc_macro'], SUM_RTOL)
        assert res[f'{t}_uauc_users'] == host['users'] and res[f'{t}_uauc_impressions'] == host['impressions']


def test_trainer_and_evaluator_report_uauc(dev):
    cfg = small_criteo('head')
    batches = _batches(cfg, 3)
    tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    assert tr.val_grouped is None and tr.train_grouped is None
    tr.enable_metrics(group_feature=FEATURE)
    probs = [tr.val_step(b)['probs'].cpu().numpy() for b in batches]
    G, Y, P = _records(batches, probs, cfg.tasks)
    res = tr.metric_results(tr.val_metrics)
    assert {f'{t}_{k}' for t in cfg.tasks for k in UAUC_KEYS} <= set(res) and 'ctr_auc' in res
    _check_against_host(res, G, Y, P, cfg.tasks)
    assert tr.train_grouped.count == 0                    # the two logs are separate
    ev = OneTransEvaluator(tr.model, cfg, group_feature=FEATURE).evaluate_offline(batches)
    _check_against_host(ev, G, Y, P, cfg.tasks)
    for t in cfg.tasks:
        for k in UAUC_KEYS:
            assert R.rel_close(ev[f'{t}_{k}'], res[f'{t}_{k}'], SUM_RTOL), (t, k)
    # a batch without the feature is refused with a clear message
    ns = {k: v for k, v in batches[0][0].items() if k != FEATURE}
    tr.group_feature = 'user_id'
    with pytest.raises(KeyError, match='user_id'):
        tr.val_step((batches[0][0], batches[0][1], batches[0][2]))
    tr.group_feature = FEATURE
    with pytest.raises(KeyError, match=FEATURE):
        tr._group_ids(ns)


def test_without_a_group_feature_nothing_changes(dev):
    cfg = small_criteo('head')
    batches = _batches(cfg, 2)
    tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    tr.enable_metrics()
    assert tr.train_grouped is None and tr.val_grouped is None
    tr.train_step(batches[0])
    tr.val_step(batches[1])
    for m in (tr.train_metrics, tr.val_metrics):
        assert not any('uauc' in k for k in tr.metric_results(m))
    ev = OneTransEvaluator(tr.model, cfg).evaluate_offline(batches)
    assert not any('uauc' in k for k in ev)
    # a second enable_metrics() without the feature switches the grouped logs off again
    tr.enable_metrics(group_feature=FEATURE)
    assert tr.val_grouped is not None
    tr.enable_metrics()
    assert tr.val_grouped is None and tr.group_feature is None


def test_fit_reports_and_resets_the_grouped_states(dev, tmp_path):
    cfg = small_criteo('head')
    batches = _batches(cfg, 3)
    tr = OneTransTrainer(cfg, model_dir=str(tmp_path), model=OneTransModel(cfg, device=dev, seed=0))
    tr.enable_metrics(group_feature=FEATURE)
    hist = tr.fit(batches[:2], batches[2:], epochs=2, save_freq=5)
    for which, nrec in (('train_metrics', 48), ('val_metrics', 24)):
        for ep in (0, 1):
            m = hist[which][ep]
            assert {f'{t}_{k}' for t in cfg.tasks for k in UAUC_KEYS} <= set(m) and 'ctr_auc' in m
            # every epoch counts its own records only: the logs were reset with the other states
            assert 0 <= m['ctr_uauc_impressions'] <= nrec and 0.0 <= m['ctr_uauc'] <= 1.0
    assert hist['train_metrics'][0]['ctr_uauc_impressions'] > 0
    assert tr.train_grouped.count == 0 and tr.val_grouped.count == 0


def test_progressive_validation_equals_the_manual_sequence(dev):
    cfg = small_criteo('head')
    batches = _batches(cfg, 4)
    period_of = lambda i, b: f'day{i // 2}'
    tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    tr.enable_metrics(group_feature=FEATURE)
    out = tr.progressive_validation(batches, period_of)
    assert list(out['periods']) == ['day0', 'day1']

    tr2 = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    tr2.enable_metrics(group_feature=FEATURE)
    manual = {}
    for d in (0, 1):
        probs = []
        for b in batches[2 * d:2 * d + 2]:
            probs.append(tr2.val_step(b)['probs'].cpu().numpy())
            tr2.train_step(b)
        manual[f'day{d}'] = tr2.metric_results(tr2.val_metrics)
        G, Y, P = _records(batches[2 * d:2 * d + 2], probs, cfg.tasks)
        _check_against_host(manual[f'day{d}'], G, Y, P, cfg.tasks)
        tr2.val_metrics.reset_states()
        tr2.val_grouped.reset_states()
    for name in manual:
        _same(out['periods'][name], manual[name])
    for k, v in out['macro'].items():
        assert v == float(np.mean([manual['day0'][k], manual['day1'][k]])), k
    a, b = tr.model.param_dict(), tr2.model.param_dict()
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # without period_of: one period
    tr3 = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, seed=0))
    one = tr3.progressive_validation(batches[:2])
    assert list(one['periods']) == [0] and 'ctr_auc' in one['macro'] and not any('uauc' in k for k in one['macro'])
    _same({k: v for k, v in out['periods']['day0'].items() if 'uauc' not in k}, one['periods'][0])
