"""CPU: the host estimator ``metrics.uauc`` against the pair-counting yardstick (grouped_auc_ref), the argument checks
of ``ot_grouped_auc`` (no device work), and the state handling of ``GroupedAUC`` on a CPU device, the 2-rank gather
included."""

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from recommend_amd import _lib
from recommend_amd.metrics import GroupedAUC, auc, uauc

import grouped_auc_ref as R

built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='library not built')


@pytest.mark.parametrize('name', list(R.CASES))
def test_uauc_equals_the_yardstick(name):
    g, y, s, _, binary, refs = R.case(name)
    for t, ref in enumerate(refs):
        if ref is None:
            continue
        got = uauc(g, y[t], s[t])
        assert np.array_equal(got['groups'], ref['ids'])
        assert np.array_equal(got['group_stats'], ref['stats'])
        assert got['users'] == ref['users'] and got['impressions'] == ref['impressions']
        assert R.rel_close(got['uauc'], ref['uauc'], 1e-12) and R.rel_close(got['uauc_macro'], ref['uauc_macro'], 1e-12)


def test_per_group_auc_equals_the_rank_auc():
    g, y, s, _, _, _ = R.case('zipf_crawler')
    got = uauc(g, y[0], s[0])
    checked = 0
    for u, (npos, nneg, u2) in zip(got['groups'], got['group_stats']):
        if npos > 0 and nneg > 0:
            m = g == u
            assert abs(u2 / (2.0 * npos * nneg) - auc(y[0][m], s[0][m])) < 1e-12
            checked += 1
    assert checked == got['users'] > 10


def test_special_values_follow_the_rule():
    """-0.0 ties with +0.0; NaNs tie with each other and rank above +inf."""
    g = np.zeros(6, dtype=np.int64)
    #             pos      neg     pos     neg      pos     neg
    s = np.array([-0.0, 0.0, np.nan, np.nan, np.nan, np.inf], dtype=np.float32)
    y = np.array([1, 0, 1, 0, 1, 0], dtype=np.float32)
    # pos -0.0: ties +0.0 (1), below NaN and inf (0 + 0) -> 1;  each NaN pos: above 0.0 (2), ties NaN (1), above inf (2)
    assert uauc(g, y, s)['group_stats'].tolist() == [[3, 3, 1 + 5 + 5]]
    assert R.ref_uauc(g, y, s)['stats'].tolist() == [[3, 3, 11]]


def test_single_class_groups_change_nothing():
    g, y, s, _, _, _ = R.case('zipf_crawler')
    base = uauc(g, y[0], s[0])
    extra = 40
    g2 = np.concatenate([g, np.full(extra, 10 ** 6), np.full(extra, 10 ** 6 + 1)])
    y2 = np.concatenate([y[0], np.ones(extra, np.float32), np.zeros(extra, np.float32)])
    s2 = np.concatenate([s[0], np.linspace(0, 1, 2 * extra, dtype=np.float32)])
    got = uauc(g2, y2, s2)
    for k in ('uauc', 'uauc_macro', 'users', 'impressions'):
        assert got[k] == base[k], k
    assert len(got['groups']) == len(base['groups']) + 2


def test_no_valid_group_reports_zero():
    g, y, s, _, _, refs = R.case('all_distinct')
    got = uauc(g, y[0], s[0])
    assert got['uauc'] == 0.0 and got['uauc_macro'] == 0.0 and got['users'] == 0 and got['impressions'] == 0
    assert refs[0]['users'] == 0
    assert uauc([], [], [])['users'] == 0


@built
def test_argument_errors_are_reported_not_crashing():
    """Invalid arguments return OT_ERR_INVALID_ARG with a message naming the function (no device work)."""
    p, ws = 4096, 1 << 30                # stand-ins for aligned device pointers: never dereferenced

    def call(groups=p, T=2, n=100, stride=100, bits=64, ws_bytes=ws):
        _lib.call('ot_grouped_auc', groups, p, p, T, n, stride, bits, 3, p, p, None, None, p, ws_bytes, None)

    with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: null operand'):
        call(groups=None)
    for T in (0, 33):
        with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: 1..32 tasks'):
            call(T=T)
    for n in (0, 1 << 31):
        with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: n out of range'):
            call(n=n, stride=1 << 31)
    with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: task_stride < n'):
        call(stride=99)
    for bits in (0, 65):
        with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: group_bits'):
            call(bits=bits)
    with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: misaligned'):
        _lib.call('ot_grouped_auc', p, p + 2, p, 2, 100, 100, 64, 3, p, p, None, None, p, ws, None)
    with pytest.raises(_lib.OneTransHipError, match='ot_grouped_auc: workspace too small'):
        call(ws_bytes=64)


@built
def test_workspace_size_grows_with_n():
    sizes = [_lib.size('ot_grouped_auc_workspace_size', 2, n, 64) for n in (1, 63, 4096, 10007, 1 << 22)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] >= (1 << 22) * 40
    assert _lib.size('ot_grouped_auc_workspace_size', 0, 100, 64) == 0
    assert _lib.size('ot_grouped_auc_workspace_size', 2, 100, 65) == 0


def test_grouped_auc_holds_state_on_a_cpu_device():
    g, y, s, _, _, _ = R.case('ties')
    m = GroupedAUC(['ctr', 'cvr', 'watch_time'], 'cpu', capacity=64)
    empty = m.result(per_group=True)
    assert empty['ctr_uauc'] == 0.0 and empty['cvr_uauc_macro'] == 0.0 and empty['ctr_uauc_users'] == 0
    assert empty['cvr_uauc_impressions'] == 0 and len(empty['groups']) == 0 and empty['ctr_group_stats'].shape == (0, 3)
    assert not any(k.startswith('watch_time') for k in empty)
    y3, s3 = np.concatenate([y, y[:1]]), np.concatenate([s, s[:1]])
    m.load_state(np.array(g), y3, s3)                                   # 257 records into a log of 64: it grows
    gs, ys, ss = m.state()
    assert m.capacity >= 257 and gs.shape == (257,) and ys.shape == ss.shape == (3, 257)
    assert np.array_equal(gs.numpy(), g) and np.array_equal(ys.numpy(), y3)
    assert ss.numpy().tobytes() == s3.tobytes()               # NaNs and signed zeros kept bit for bit
    with pytest.raises(_lib.OneTransHipError, match='GPU only'):
        m.update(torch.from_numpy(np.array(g)), torch.from_numpy(y3), torch.from_numpy(s3))
    with pytest.raises(_lib.OneTransHipError, match='GPU only'):
        m.result()
    m.reset_states()
    assert m.state()[0].numel() == 0 and m.result()['ctr_uauc'] == 0.0


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _parts():
    g, y, s, _, _, _ = R.case('ties')
    cut = lambda a, b: tuple(np.array(x[..., a:b]) for x in (g, y, s))
    return [cut(0, 100), cut(100, 257)]


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        m = GroupedAUC(['ctr', 'cvr'], 'cpu', capacity=128)
        m.load_state(*_parts()[rank])
        m.all_gather()
        q.put((rank,) + tuple(t.numpy().tobytes() for t in m.state()))
    finally:
        dist.destroy_process_group()


def test_all_gather_leaves_every_rank_with_all_records():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    g, y, s, _, _, _ = R.case('ties')
    assert sorted(r[0] for r in got) == [0, 1]
    for _, gs, ys, ss in got:
        assert gs == g.tobytes() and ys == y.tobytes() and ss == s.tobytes()


def test_all_gather_is_a_no_op_outside_a_process_group():
    m = GroupedAUC(['ctr'], 'cpu', capacity=8)
    m.load_state([1, 2, 3], [[1, 0, 1]], [[0.1, 0.2, 0.3]])
    m.all_gather()
    assert m.state()[0].tolist() == [1, 2, 3]
