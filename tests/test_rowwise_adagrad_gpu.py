"""Row-wise Adagrad for the embedding tables (``optimizer_config['sparse_optimizer'] = 'rowwise_adagrad'``) on the
GPU: the three kernels' forms through the C ABI against the float64 reference (tests/rowwise_ref.py) and against
each other, the exact tie to the untouched element-wise kernel, and the trainer: one step, a resumed run and a table
row-sharded over two ranks.

Inputs of the kernel tests: table_ref.table_inputs(E) (400 rows, ~1500 pairs, a hot key with a run of 200, five
invalid keys), accumulators [400] at 0.1, LR and EPS of table_ref.  Tolerances: rowwise_ref.W_TOL / A_TOL (table
rtol 1e-5 / atol 1e-6, accumulator rtol 1e-5 / atol 1e-5), which tests/test_rowwise_adagrad.py shows an f32
restatement of the update to meet at every width.

Row widths: a row gets tps = min(E / 4, 64) threads of a 256-thread block.  WIDTHS holds one lane per row (4),
groups that straddle a wavefront boundary (12, 20, 24, 40, 48, 96, 192: tps is no power of two), whole-wavefront
groups with one column pass (256) and with several, the last one partial (252 is one short pass; 520, 1024)."""

import os
import queue
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import release_device_cache
from recommend_amd import kernels as K
from recommend_amd.data import make_batch
from recommend_amd.model import OneTransModel
from recommend_amd.params import init_params
from recommend_amd.trainer import OneTransTrainer
from rowwise_ref import A_TOL, W_TOL, rowwise_adagrad_ref
from table_ref import EPS, LR, NUM_ROWS, table_inputs

from test_model_gpu import small_criteo

WIDTHS = [4, 12, 16, 20, 24, 40, 48, 64, 96, 192, 252, 256, 520, 1024]
ROWWISE = 'rowwise_adagrad'


def _bits(x):
    a = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint32)


def _device_inputs(E, dev):
    """table_inputs(E) with the accumulator per row: host (keys, grads, table, accum_rows, valid unique keys) and
    device (keys, grads, table, accum_rows)."""
    keys, grads, table, accum = table_inputs(E)
    a0 = np.ascontiguousarray(accum[:, 0])
    uk = np.unique(keys[(keys >= 0) & (keys < NUM_ROWS)])
    return (keys, grads, table, a0, uk) + tuple(torch.tensor(a, device=dev) for a in (keys, grads, table, a0))


def _one_call(E, dev, clip):
    keys, grads, table, a0, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    K.sparse_adagrad_rowwise(t_d, a_d, E, NUM_ROWS, k_d, g_d, len(keys), LR, EPS, clip, device=dev)
    return t_d, a_d


def _two_phase(E, dev, clip):
    keys, grads, table, a0, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    n = len(keys)
    ws = K.sparse_workspace(n, E, dev)
    sumsq = torch.zeros(1, device=dev)
    K.sparse_prepare(E, NUM_ROWS, k_d, g_d, n, sumsq, ws)
    K.sparse_finish_rowwise(t_d, a_d, E, n, LR, EPS, clip, sumsq, ws)      # prepare's own norm
    return t_d, a_d


def _dense_form(E, dev, clip):
    keys, grads, table, a0, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    dense = torch.zeros(NUM_ROWS, E, device=dev)
    K.sparse_grad_dense(E, NUM_ROWS, k_d, g_d, len(keys), dense, device=dev)
    K.dense_adagrad_rowwise(t_d, a_d, dense, NUM_ROWS, E, LR, EPS, clip, device=dev)
    return t_d, a_d


FORMS = {'one_call': _one_call, 'two_phase': _two_phase, 'dense': _dense_form}


# ------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('clip', [0.0, 3.0, 1e6])
@pytest.mark.parametrize('E', WIDTHS)
def test_rowwise_vs_float64(dev, E, clip):
    """ot_sparse_adagrad_rowwise, one call, against the float64 reference with the clip off (0), active (3: the
    gradient norm is ~sqrt(1500 E)) and inactive (1e6)."""
    keys, grads, table, a0, uk = _device_inputs(E, dev)[:5]
    w_ref, a_ref, uk_ref = rowwise_adagrad_ref(table, a0, keys, grads, NUM_ROWS, LR, EPS, clip)
    assert np.array_equal(uk, uk_ref)
    t_d, a_d = _one_call(E, dev, clip)
    w, a = t_d.cpu().numpy(), a_d.cpu().numpy()
    assert a.shape == (NUM_ROWS,)
    np.testing.assert_allclose(w, w_ref, **W_TOL)
    np.testing.assert_allclose(a, a_ref, **A_TOL)
    assert np.abs(w - table)[uk].max() > 1e-4 and (a[uk] > a0[uk]).all()
    again = _one_call(E, dev, clip)                                  # no atomics: the same bits run to run
    assert torch.equal(again[0], t_d) and torch.equal(again[1], a_d)


# ------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('E', [4, 16, 64, 256, 1024])
def test_rowwise_ties_to_elementwise_kernel(dev, E):
    """Unique keys, every gradient entry of row r = +-2^-k_r, clip off: a row's squares are all 4^-k_r, every sum of
    them is exact in any order and their mean is 4^-k_r again, so the row-wise update IS the element-wise one.  The
    table equals the untouched ot_sparse_adagrad's bit for bit and the row accumulator equals every column of the
    element-wise accumulator.  A lane that reads another row's columns, skips a pass or counts one twice changes the
    mean and fails."""
    rng = np.random.default_rng(50 + E)
    rows = 300
    keys = rng.permutation(NUM_ROWS)[:rows].astype(np.int64)        # unique, unsorted
    k_r = rng.integers(0, 12, rows)
    grads = (np.ldexp(1.0, -k_r)[:, None] * rng.choice([-1.0, 1.0], (rows, E))).astype(np.float32)
    table = rng.uniform(-0.05, 0.05, (NUM_ROWS, E)).astype(np.float32)
    T = lambda a: torch.tensor(a, device=dev)
    k_d, g_d = T(keys), T(grads)
    t_el, a_el = T(table), torch.full((NUM_ROWS, E), 0.1, device=dev)
    K.sparse_adagrad(t_el, a_el, E, NUM_ROWS, k_d, g_d, rows, LR, EPS, 0.0, device=dev)
    t_rw, a_rw = T(table), torch.full((NUM_ROWS,), 0.1, device=dev)
    K.sparse_adagrad_rowwise(t_rw, a_rw, E, NUM_ROWS, k_d, g_d, rows, LR, EPS, 0.0, device=dev)
    assert np.array_equal(_bits(t_rw), _bits(t_el))
    assert np.array_equal(_bits(a_rw)[:, None].repeat(E, 1), _bits(a_el))
    assert (a_rw.cpu().numpy()[keys] > np.float32(0.1)).all() and not np.array_equal(_bits(t_rw), _bits(table))
    # the dense form from the same rows: the same bits again
    dense = torch.zeros(NUM_ROWS, E, device=dev)
    K.sparse_grad_dense(E, NUM_ROWS, k_d, g_d, rows, dense, device=dev)
    t_dn, a_dn = T(table), torch.full((NUM_ROWS,), 0.1, device=dev)
    K.dense_adagrad_rowwise(t_dn, a_dn, dense, NUM_ROWS, E, LR, EPS, 0.0, device=dev)
    assert np.array_equal(_bits(t_dn), _bits(t_el)) and np.array_equal(_bits(a_dn), _bits(a_rw))


# ------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('clip', [0.0, 3.0])
@pytest.mark.parametrize('E', WIDTHS)
def test_forms_agree(dev, E, clip):
    """ot_sparse_prepare + ot_sparse_finish_rowwise (fed prepare's own norm) and ot_sparse_grad_dense +
    ot_dense_adagrad_rowwise against the one call.  With the clip off nothing differs between the forms but the
    kernel that applies the rule, and the row's sum of squares is added in an order fixed by E: the same bits."""
    t1, a1 = _one_call(E, dev, clip)
    for name in ('two_phase', 'dense'):
        t2, a2 = FORMS[name](E, dev, clip)
        torch.testing.assert_close(t2, t1, msg=lambda m: f'{name}: {m}', **W_TOL)
        torch.testing.assert_close(a2, a1, msg=lambda m: f'{name}: {m}', **A_TOL)
        if clip == 0.0:
            assert torch.equal(t2, t1) and torch.equal(a2, a1), name


# ------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('E', [4, 12, 64, 252, 1024])
def test_untouched_state(dev, E):
    """Rows no valid key names keep weight and accumulator bits in all three forms; n = 0 (dense: an all-zero
    gradient) writes nothing."""
    keys, grads, table, a0, uk, k_d, g_d, t_d, a_d = _device_inputs(E, dev)
    rest = np.setdiff1d(np.arange(NUM_ROWS), uk)
    assert len(rest) >= 20
    for name, form in FORMS.items():
        t, a = form(E, dev, 3.0)
        assert np.array_equal(_bits(t)[rest], _bits(table)[rest]), name
        assert np.array_equal(_bits(a)[rest], _bits(a0)[rest]), name
        assert not np.array_equal(_bits(a)[uk], _bits(a0)[uk]), name
    K.sparse_adagrad_rowwise(t_d, a_d, E, NUM_ROWS, k_d, g_d, 0, LR, EPS, 3.0, device=dev)
    ws = torch.full((256,), 0xAB, dtype=torch.uint8, device=dev)
    K.sparse_finish_rowwise(t_d, a_d, E, 0, LR, EPS, 3.0, torch.ones(1, device=dev), ws)
    assert bool((ws == 0xAB).all())
    K.dense_adagrad_rowwise(t_d, a_d, torch.zeros(NUM_ROWS, E, device=dev), NUM_ROWS, E, LR, EPS, 3.0, device=dev)
    assert np.array_equal(_bits(t_d), _bits(table)) and np.array_equal(_bits(a_d), _bits(a0))


# ------------------------------------------------------------------------------------------------- trainer
def _config(kind):
    cfg = small_criteo('tail', pyramid=True, layers=3)
    cfg.dropout_rate = 0.0
    cfg.optimizer_config = dict(cfg.optimizer_config, sparse_optimizer=kind)
    return cfg


def _trainer(dev, kind, tmp_path=None, seed=None):
    cfg = _config(kind)
    if seed is None:
        model = OneTransModel(cfg, device=dev, init=init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True))
    else:
        model = OneTransModel(cfg, device=dev, seed=seed)
    return cfg, OneTransTrainer(cfg, model_dir=str(tmp_path or './models'), model=model)


def test_trainer_step(dev):
    """One train_step under 'rowwise_adagrad': every table against the float64 reference applied to the (key,
    gradient row) pairs the step itself queued (copied just before optimizer.step()); the dense parameters bit for
    bit those of an 'adagrad' trainer from the same init and batch; the optimizer state smaller by exactly
    sum over the tables of rows (E - 1) 4 bytes."""
    cfg, tr = _trainer(dev, ROWWISE)
    _, tr_el = _trainer(dev, 'adagrad')
    opt = tr.optimizer
    assert opt.sparse_kind == ROWWISE and tr_el.optimizer.sparse_kind == 'adagrad'
    saved = sum(t.shape[0] * (t.shape[1] - 1) * 4 for t in tr.model.tables.values())
    assert saved > 0 and tr_el.optimizer.state_nbytes() - opt.state_nbytes() == saved
    assert tr_el.optimizer.state_nbytes() == 4 * (2 * tr.model.flat.numel()
                                                  + sum(t.numel() for t in tr.model.tables.values()))
    for name, t in tr.model.tables.items():
        assert opt.acc[name].shape == (t.shape[0],)
    before = {k: (t.cpu().numpy().copy(), opt.acc[k].cpu().numpy().copy()) for k, t in tr.model.tables.items()}
    captured = []
    real_step = opt.step

    def step():
        captured.extend((n, k.detach().cpu().numpy().reshape(-1), g.detach().cpu().numpy().reshape(-1, g.shape[-1]))
                        for (n, k, g) in tr.model._pending_sparse)
        real_step()

    opt.step = step
    batch = make_batch(16, cfg, seed=7)
    tr.train_step(batch)
    tr_el.train_step(batch)
    assert {n for n, _, _ in captured} == set(tr.model.tables)
    for name, table in tr.model.tables.items():
        keys = np.concatenate([k for n, k, _ in captured if n == name])
        grads = np.concatenate([g for n, _, g in captured if n == name])
        w0, a0 = before[name]
        w_ref, a_ref, uk = rowwise_adagrad_ref(w0, a0, keys, grads, table.shape[0], opt.sparse_lr, opt.sparse_eps,
                                               opt.sparse_clip)
        w, a = table.cpu().numpy(), opt.acc[name].cpu().numpy()
        np.testing.assert_allclose(w, w_ref, err_msg=name, **W_TOL)
        np.testing.assert_allclose(a, a_ref, err_msg=name, **A_TOL)
        assert np.abs(w - w0).max() > 1e-5, name
        rest = np.setdiff1d(np.arange(table.shape[0]), uk)
        assert np.array_equal(_bits(w[rest]), _bits(w0[rest])) and np.array_equal(_bits(a[rest]), _bits(a0[rest]))
    assert torch.equal(tr.model.flat.data, tr_el.model.flat.data)
    assert not torch.equal(tr.model.tables['emb.seq_item'], tr_el.model.tables['emb.seq_item'])


def test_unknown_sparse_optimizer_is_refused(dev):
    cfg = _config('ftrl')
    model = OneTransModel(cfg, device=dev, seed=1)
    with pytest.raises(ValueError, match='sparse_optimizer'):
        OneTransTrainer(cfg, model=model)


def test_resume(dev, tmp_path):
    """Two steps, save_model with the optimizer state, load_model into a fresh trainer, step three: tables,
    accumulators and dense weights bitwise those of the uninterrupted run.  A state of the other sparse kind is
    refused whole; a state without 'sparse_kind' is an 'adagrad' state."""
    cfg, tr = _trainer(dev, ROWWISE, tmp_path)
    batches = [make_batch(16, cfg, seed=7 + i) for i in range(3)]
    for b in batches[:2]:
        tr.train_step(b)
    tr.save_model('ck', include_optimizer=True)
    state = tr.optimizer.state_dict()
    assert str(state['sparse_kind']) == ROWWISE
    for name, t in tr.model.tables.items():
        assert state[f'acc.{name}'].shape == (t.shape[0],)
        assert (state[f'acc.{name}'] != np.float32(cfg.adagrad_initial_accumulator)).any()

    _, tr2 = _trainer(dev, 'adagrad', tmp_path, seed=5)              # load_model takes the kind from config.json
    tr2.load_model(str(tmp_path / 'ck'))
    assert tr2.optimizer.sparse_kind == ROWWISE and tr2.optimizer.steps_done == 2
    tr.train_step(batches[2])
    tr2.train_step(batches[2])
    assert torch.equal(tr2.model.flat.data, tr.model.flat.data)
    for k in tr.model.tables:
        assert torch.equal(tr2.model.tables[k], tr.model.tables[k]), k
        assert torch.equal(tr2.optimizer.acc[k], tr.optimizer.acc[k]), k

    # an 'adagrad' state into a row-wise optimizer, and the reverse: ValueError, nothing written
    _, tr_el = _trainer(dev, 'adagrad', tmp_path)
    tr_el.train_step(batches[0])
    el_state = tr_el.optimizer.state_dict()
    assert 'sparse_kind' not in el_state                             # the keys an 'adagrad' state always had
    _, tr3 = _trainer(dev, ROWWISE, tmp_path, seed=5)
    acc0 = {k: a.clone() for k, a in tr3.optimizer.acc.items()}
    with pytest.raises(ValueError, match="sparse optimizer 'adagrad'"):
        tr3.optimizer.load_state_dict(el_state)
    with pytest.raises(ValueError, match="sparse optimizer 'rowwise_adagrad'"):
        tr_el.optimizer.load_state_dict(state)
    wrong = dict(state)
    wrong['acc.emb.seq_item'] = np.repeat(state['acc.emb.seq_item'][:, None], cfg.seq_feature_dim, 1)
    with pytest.raises(ValueError, match='acc.emb.seq_item'):
        tr3.optimizer.load_state_dict(wrong)
    assert tr3.optimizer.steps_done == 0 and not tr3.optimizer.v.any() and not tr3.optimizer.m.any()
    for k, a in tr3.optimizer.acc.items():
        assert torch.equal(a, acc0[k]), k
    assert tr_el.optimizer.steps_done == 1

    # no 'sparse_kind' (a checkpoint from before the switch): an 'adagrad' state
    old = dict(el_state)
    old.pop('sparse_kind', None)
    _, tr4 = _trainer(dev, 'adagrad', tmp_path, seed=5)
    tr4.optimizer.load_state_dict(old)
    assert tr4.optimizer.steps_done == 1
    for k in tr_el.model.tables:
        assert torch.equal(tr4.optimizer.acc[k], tr_el.optimizer.acc[k]), k
    stripped = {k: v for k, v in state.items() if k != 'sparse_kind'}
    with pytest.raises(ValueError, match="sparse optimizer 'adagrad'"):      # ... and so no row-wise one
        tr3.optimizer.load_state_dict(stripped)


# ------------------------------------------------------------------------------------------------- row-sharded
SHARD_B, SHARD_STEPS = 40, 3


def _shard_config():
    cfg = small_criteo('head', d=64, H=4, f=128, Lns=4, seq_lens=(5, 9, 7))      # test_sharded_gpu's
    cfg.dropout_rate = 0.0
    cfg.optimizer_config = dict(cfg.optimizer_config, dense_lr=0.001, momentum=0.9, sparse_optimizer=ROWWISE)
    return cfg


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['ONETRANS_TABLE_SHARDING'] = 'row'
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        dev = torch.device('cuda:0')
        cfg = _shard_config()
        model = OneTransModel(cfg, device=dev, init=init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True))
        st = model.sharded['emb.seq_item']
        tr = OneTransTrainer(cfg, model=model)
        assert tr.optimizer.acc['emb.seq_item'].shape == (st.rows_alloc,)
        sl = slice(rank * SHARD_B // world, (rank + 1) * SHARD_B // world)
        for step in range(SHARD_STEPS):
            batch = make_batch(SHARD_B, cfg, seed=3000 + step)
            tr.train_step(tuple({k: v[sl] for k, v in x.items()} for x in batch))
        params = model.param_dict()                      # collectives: every rank calls them
        state = tr.optimizer.state_dict()
        if rank == 0:
            q.put((params, state))
    finally:
        dist.destroy_process_group()


def test_row_sharded_two_ranks(dev):
    """Three data-parallel steps with 'emb.seq_item' row-sharded over two ranks (one GPU, gloo, as
    tests/test_sharded_gpu.py sets it up; the replicated emb.ns takes the dense exchange, ot_dense_adagrad_rowwise)
    against the single-process replicated row-wise run on the full batch, at that file's bound for the same
    comparison under 'adagrad' (2e-4, every parameter and the logical table).  The gathered [rows] accumulators are
    compared too, at the same bound, and name the same rows as touched."""
    import torch.multiprocessing as mp
    cfg = _shard_config()
    model = OneTransModel(cfg, device=dev, init=init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True))
    assert not model.sharded
    tr = OneTransTrainer(cfg, model=model)
    for step in range(SHARD_STEPS):
        tr.train_step(make_batch(SHARD_B, cfg, seed=3000 + step))
    ref_params, ref_state = model.param_dict(), tr.optimizer.state_dict()
    del tr, model
    release_device_cache()

    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    env_pp = os.environ.get('PYTHONPATH', '')
    here = os.path.dirname(os.path.abspath(__file__))
    os.environ['PYTHONPATH'] = os.pathsep.join([here, os.path.dirname(here)] + ([env_pp] if env_pp else []))
    try:
        procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        result = None                                    # taken before the joins (a queue's feeder blocks on large
        for _ in range(120):                             # items); given up as soon as a rank has failed
            try:
                result = q.get(timeout=2)
                break
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):
                    break
        for p in procs:
            p.join(60 if result is not None else 5)
    finally:
        os.environ['PYTHONPATH'] = env_pp
        for p in procs:
            if p.exitcode is None:
                p.kill()
    for p in procs:
        assert p.exitcode == 0, p.exitcode
    assert result is not None
    params, state = result
    assert set(params) == set(ref_params) and set(state) == set(ref_state)
    bad = {k: float(np.abs(params[k] - v).max()) for k, v in ref_params.items() if np.abs(params[k] - v).max() >= 2e-4}
    assert not bad, bad
    init = np.float32(cfg.adagrad_initial_accumulator)
    for name in ('emb.seq_item', 'emb.ns'):
        a, r = state[f'acc.{name}'], ref_state[f'acc.{name}']
        assert a.shape == r.shape == (ref_params[name].shape[0],)
        assert np.abs(a - r).max() < 2e-4, name
        assert np.array_equal(a != init, r != init) and (a != init).sum() > 10, name
    assert str(state['sparse_kind']) == ROWWISE
