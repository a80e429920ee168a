"""The Adam dense optimizer on the GPU: ot_clip_adam against the float64 reference (tests/adam_ref.py), its edge
cases and determinism, the trainer's choice of optimizer from ``optimizer_config['dense_optimizer']``
(train.py:53-76) and the resumable optimizer state (``save_model(..., include_optimizer=True)``).

Tolerances are test_kernels_gpu.test_clip_rmsprop's, the same arithmetic class (an f32 clip scale from a
fixed-order sum of squares, then a handful of f32 operations per element): w rtol 1e-5 / atol 1e-6, the two
slots rtol 1e-5 / atol 1e-7.

The reference gets the hyper-parameters as the C ABI carries them, rounded to float32 (``_f32``), like the float32
buffers it is given: ot_clip_adam takes lr / beta1 / beta2 / eps as ``float``, and Keras casts them to the
variable's float32 as well.  It matters for beta2 only: float32(0.999) is 0.99900001287, so 1 - beta2 is
0.00099998713, 1.29e-5 (relative) off 0.001 -- more than the rtol, in every v increment, before the kernel has
done any arithmetic (measured with the unrounded 0.999: 2 of 5,200 v elements at 1.28e-5 relative)."""

import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adam_ref
from oracle import keras_math as km
from recommend_amd import kernels as K
from recommend_amd._lib import OneTransHipError
from recommend_amd.data import make_batch
from recommend_amd.model import OneTransModel
from recommend_amd.params import init_params
from recommend_amd.trainer import OneTransTrainer

from test_model_gpu import small_criteo


def _f32(x):
    """A hyper-parameter as a ``float`` argument of the C ABI holds it."""
    return float(np.float32(x))


W_TOL = dict(rtol=1e-5, atol=1e-6)
S_TOL = dict(rtol=1e-5, atol=1e-7)

TOTAL = 5200
# two interleaved column slices of one bank; one row longer than a 4,096-element chunk by a non-multiple of 4 at
# an offset that is no multiple of 4; a contiguous 16-byte aligned segment (the vector path); a small strided
# segment (its gradient is zero below); gaps at 600, 4700..4703, inside the last segment's rows and after it
SEGS = np.array([[0, 10, 30, 60], [30, 10, 30, 60], [601, 1, 4099, 4099], [4704, 20, 20, 20], [5104, 3, 7, 9]],
                np.int64)
MAX_SEG = 4099
G_SCALE = [10.0, 0.1, 10.0, 0.05, 0.0]      # per segment: the clip of 50 bites on 0 and 2 only
LR, B1, B2, EPS, CLIP = 0.005, 0.9, 0.999, 1e-7, 50.0


def _covered():
    c = np.zeros(TOTAL, bool)
    for seg in SEGS:
        c[adam_ref.seg_index(seg)] = True
    return c


def _state(seed):
    """float32 host buffers (w, g, m, v): nonzero moments, per-segment gradient scales, junk in the gaps."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=TOTAL)
    g = rng.normal(size=TOTAL)                  # (uncovered gradient entries stay ~N(0, 1): they must be ignored)
    for seg, s in zip(SEGS, G_SCALE):
        g[adam_ref.seg_index(seg)] *= s
    m = rng.normal(size=TOTAL) * 0.01
    v = np.abs(rng.normal(size=TOTAL)) * 0.01
    return [a.astype(np.float32) for a in (w, g, m, v)]


def _run(dev, w, g, m, v, step, lr=LR, beta1=B1, beta2=B2, eps=EPS, clip=CLIP):
    """ot_clip_adam on device copies -> (w, m, v) device tensors."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    wd, gd, md, vd = T(w), T(g), T(m), T(v)
    K.clip_adam(wd, gd, md, vd, T(SEGS.reshape(-1)), len(SEGS), MAX_SEG, lr, beta1, beta2, eps, step, clip,
                device=dev)
    return wd, md, vd


def _check(got, before, g, step, **kw):
    """(w, m, v) from the device against adam_ref on the same float32 inputs; uncovered elements bit-identical."""
    w, m, v = before
    args = dict(lr=LR, beta1=B1, beta2=B2, eps=EPS, clip=CLIP)
    args.update(kw)
    rw, rm, rv = adam_ref.clip_adam(w, g, m, v, SEGS, step=step, **{k: _f32(x) for k, x in args.items()})
    gw, gm, gv = (t.cpu().numpy() for t in got)
    np.testing.assert_allclose(gw, rw, **W_TOL)
    np.testing.assert_allclose(gm, rm, **S_TOL)
    np.testing.assert_allclose(gv, rv, **S_TOL)
    un = ~_covered()
    assert un.sum() > 50
    for a, b in ((gw, w), (gm, m), (gv, v)):
        assert np.array_equal(a[un].view(np.uint32), b[un].view(np.uint32))
    return gw, gm, gv


def test_clip_adam_vs_float64(dev):
    w, g, m, v = _state(11)
    norms = [float(np.linalg.norm(g[adam_ref.seg_index(s)].astype(np.float64))) for s in SEGS]
    assert norms[0] > CLIP and norms[2] > CLIP and 0 < norms[1] < CLIP and 0 < norms[3] < CLIP and norms[4] == 0
    rng = np.random.default_rng(12)
    for step in (1, 2, 3):                       # each step checked from the state the device left
        got = _run(dev, w, g, m, v, step)
        w, m, v = _check(got, (w, m, v), g, step)
        assert np.isfinite(w).all() and np.isfinite(m).all() and np.isfinite(v).all()
        g = (g * rng.uniform(0.5, 1.5, size=TOTAL)).astype(np.float32)
    # the step argument is used: the same state at step 1000 (bias corrections 0.632 and 1, not 0.001 and 0.1)
    w, g, m, v = _state(13)
    got = _run(dev, w, g, m, v, 1000)
    w1000 = _check(got, (w, m, v), g, 1000)[0]
    w1 = _run(dev, w, g, m, v, 1)[0].cpu().numpy()
    assert np.abs(w1000 - w1)[_covered()].max() > 1e-4


def test_clip_adam_edge_cases(dev):
    w, g, m, v = _state(21)
    # clip = 0: no clipping
    _check(_run(dev, w, g, m, v, 2, clip=0.0), (w, m, v), g, 2, clip=0.0)
    # beta2 = 1 (the reference's default optimizer_config): alpha = 0 -- w and v keep their bits, m moves
    gw, gm, gv = _check(_run(dev, w, g, m, v, 5, beta1=0.1, beta2=1.0), (w, m, v), g, 5, beta1=0.1, beta2=1.0)
    assert np.array_equal(gw.view(np.uint32), w.view(np.uint32)) and np.array_equal(gv.view(np.uint32),
                                                                                    v.view(np.uint32))
    assert np.isfinite(gw).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
    big = adam_ref.seg_index(SEGS[2])
    assert np.abs(gm - m)[big].max() > 1e-3
    # ... also from v = 0 (a fresh optimizer): 0 / (0 + eps), not 0 / 0
    z = np.zeros_like(v)
    gw, gm, gv = (t.cpu().numpy() for t in _run(dev, w, g, z, z, 1, beta1=0.1, beta2=1.0))
    assert np.array_equal(gw.view(np.uint32), w.view(np.uint32)) and not gv.any() and np.isfinite(gm).all()
    # beta1 = 0: m becomes the clipped gradient
    _check(_run(dev, w, g, m, v, 3, beta1=0.0), (w, m, v), g, 3, beta1=0.0)
    # argument checks (no device work): step is 1-based, beta1 < 1, beta2 <= 1
    for bad in (dict(step=0), dict(step=1, beta1=1.0), dict(step=1, beta2=1.5), dict(step=1, beta1=-0.1)):
        with pytest.raises(OneTransHipError, match='ot_clip_adam'):
            _run(dev, w, g, m, v, **bad)
    # no segments: nothing to do
    wd = torch.from_numpy(w).to(dev)
    K.clip_adam(wd, wd.clone(), wd.clone(), wd.clone(), torch.zeros(4, dtype=torch.int64, device=dev), 0, 0, LR, B1,
                B2, EPS, 1, CLIP, device=dev)
    assert np.array_equal(wd.cpu().numpy(), w)


def test_clip_adam_deterministic(dev):
    w, g, m, v = _state(31)
    a = _run(dev, w, g, m, v, 4)
    b = _run(dev, w, g, m, v, 4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------- trainer
def _trainer(dev, tmp_path=None, seed=None, **oc):
    cfg = small_criteo('tail', pyramid=True, layers=3)
    cfg.dropout_rate = 0.0
    cfg.optimizer_config = dict(cfg.optimizer_config, **oc)
    if seed is None:
        model = OneTransModel(cfg, device=dev, init=init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True))
    else:
        model = OneTransModel(cfg, device=dev, seed=seed)
    return cfg, OneTransTrainer(cfg, model_dir=str(tmp_path or './models'), model=model)


def _step_matches_adam_ref(tr, cfg, batch, beta1, beta2, eps):
    """One train_step against adam_ref applied, per layout segment, to the gradient the step itself computed
    (step() leaves flat.grad intact at world 1) and the weights / slots snapshotted before it."""
    opt, model = tr.optimizer, tr.model
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    w0, m0, v0 = f64(model.flat.data), f64(opt.m), f64(opt.v)
    tr.train_step(batch)
    g = f64(model.flat.grad)
    assert np.abs(g).max() > 0
    rw, rm, rv = adam_ref.clip_adam(w0, g, m0, v0, model.layout.segments, _f32(cfg.optimizer_config['dense_lr']),
                                    _f32(beta1), _f32(beta2), _f32(eps), opt.steps_done,
                                    _f32(cfg.gradient_clip_norm))
    np.testing.assert_allclose(f64(model.flat.data), rw, **W_TOL)
    np.testing.assert_allclose(f64(opt.m), rm, **S_TOL)
    np.testing.assert_allclose(f64(opt.v), rv, **S_TOL)
    assert np.abs(rw - w0).max() > 1e-4                               # the step moved the weights


def test_trainer_adam_steps_match_reference(dev):
    cfg, tr = _trainer(dev, dense_optimizer='adam', beta1=0.9, beta2=0.999)
    assert tr.optimizer.kind == 'adam'
    batch = make_batch(16, cfg, seed=7)
    for i in range(3):
        _step_matches_adam_ref(tr, cfg, batch, 0.9, 0.999, 1e-8)
        assert tr.optimizer.steps_done == i + 1


def test_trainer_unknown_name_is_keras_default_adam(dev):
    """train.py:71-74: any other name gives Adam with the Keras defaults; optimizer_config's beta1 0.1 / beta2 1.0
    (the default dict's) and epsilon are not read."""
    cfg, tr = _trainer(dev, dense_optimizer='sgd', epsilon=1e-3)
    assert cfg.optimizer_config['beta1'] == 0.1 and cfg.optimizer_config['beta2'] == 1.0
    _step_matches_adam_ref(tr, cfg, make_batch(16, cfg, seed=7), 0.9, 0.999, 1e-7)


def test_trainer_default_config_still_rmsprop(dev, monkeypatch):
    cfg, tr = _trainer(dev)
    assert tr.optimizer.kind == 'rmsprop'
    calls = []
    real = K.clip_rmsprop
    monkeypatch.setattr(K, 'clip_rmsprop', lambda *a, **k: (calls.append(a[7:12]), real(*a, **k))[1])
    monkeypatch.setattr(K, 'clip_adam', lambda *a, **k: pytest.fail('clip_adam called under rmsprop'))
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    w0 = f64(tr.model.flat.data)
    tr.train_step(make_batch(16, cfg, seed=7))
    assert calls == [(0.005, 0.9, 1e-7, 0.99999, 90.0)]                # lr, rho, eps, momentum, clip: today's
    g = f64(tr.model.flat.grad)
    gc, covered = g.copy(), np.zeros(g.size, bool)
    for seg in tr.model.layout.segments:
        idx = adam_ref.seg_index(seg)
        gc[idx] = km.clip_by_norm(g[idx], 90.0)
        covered[idx] = True
    z = np.zeros_like(w0)
    w2, v2, m2 = km.rmsprop_update(w0, gc, z, z, 0.005, 0.9, 1e-7, 0.99999)
    np.testing.assert_allclose(f64(tr.model.flat.data), np.where(covered, w2, w0), **W_TOL)
    np.testing.assert_allclose(f64(tr.optimizer.v), np.where(covered, v2, 0.0), **S_TOL)
    np.testing.assert_allclose(f64(tr.optimizer.m), np.where(covered, m2, 0.0), **S_TOL)


def test_trainer_adam_learns(dev):
    cfg, tr = _trainer(dev, dense_optimizer='adam', beta1=0.9, beta2=0.999, dense_lr=1e-3)
    batch = make_batch(32, cfg, seed=9)
    losses = torch.stack([tr.train_step(batch)['total_loss'] for _ in range(20)]).cpu().numpy()
    assert np.isfinite(losses).all(), losses
    assert losses[19] < losses[0], losses


def test_resume_with_optimizer_state(dev, tmp_path):
    """A checkpoint with the optimizer state resumes bit for bit (dropout is off: the dropout step counter is no
    part of a checkpoint); one without it restores the weights as before and then steps differently."""
    adam = dict(dense_optimizer='adam', beta1=0.9, beta2=0.999)
    cfg, tr = _trainer(dev, tmp_path, **adam)
    batch = make_batch(16, cfg, seed=7)
    for _ in range(3):
        tr.train_step(batch)
    tr.save_model('ck', include_optimizer=True)
    tr.save_model('ck2')
    files = {'model_weights.npz', 'config.json', 'training_history.json'}
    assert {p.name for p in (tmp_path / 'ck').iterdir()} == files | {'optimizer_state.npz'}
    assert {p.name for p in (tmp_path / 'ck2').iterdir()} == files
    shutil.copytree(tmp_path / 'ck', tmp_path / 'ck_nostate')
    (tmp_path / 'ck_nostate' / 'optimizer_state.npz').unlink()

    _, tr2 = _trainer(dev, tmp_path, seed=5, **adam)
    tr2.load_model(str(tmp_path / 'ck'))
    assert tr2.optimizer.kind == 'adam' and tr2.optimizer.steps_done == 3
    a, b = tr.optimizer.state_dict(), tr2.optimizer.state_dict()
    assert set(a) == set(b) == {'dense_kind', 'steps_done', 'dense.v', 'dense.m'} | {f'acc.{k}' for k in
                                                                                   tr.model.tables}
    assert np.abs(a['dense.m']).max() > 0 and np.abs(a['dense.v']).max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _, tr3 = _trainer(dev, tmp_path, seed=5, **adam)
    tr3.load_model(str(tmp_path / 'ck_nostate'))                  # restoring works as before
    assert tr3.optimizer.steps_done == 3 and not tr3.optimizer.m.any()
    assert torch.equal(tr3.model.flat.data, tr.model.flat.data)

    for t in (tr, tr2, tr3):
        t.train_step(batch)
    assert torch.equal(tr2.model.flat.data, tr.model.flat.data)
    for k in tr.model.tables:
        assert torch.equal(tr2.model.tables[k], tr.model.tables[k]), k
        assert torch.equal(tr2.optimizer.acc[k], tr.optimizer.acc[k]), k
    assert not torch.equal(tr3.model.flat.data, tr.model.flat.data)   # the state file matters

    # a state of the other dense kind is refused, and nothing is restored
    _, tr4 = _trainer(dev, tmp_path, seed=5)
    with pytest.raises(ValueError, match='adam'):
        tr4.optimizer.load_state_dict(a)
    assert tr4.optimizer.steps_done == 0 and not tr4.optimizer.v.any()


def test_state_dict_row_sharded_table(dev, monkeypatch):
    """A row-sharded table's accumulator is saved as the logical table (gathered like the weights in param_dict)
    and restored into this rank's rows; here one process holds the one shard.  A state that does not fit is
    refused whole, in an error that names the entry."""
    monkeypatch.setenv('ONETRANS_TABLE_SHARDING', 'row')
    adam = dict(dense_optimizer='adam', beta1=0.9, beta2=0.999)
    cfg, tr = _trainer(dev, **adam)
    st = tr.model.sharded['emb.seq_item']
    batch = make_batch(16, cfg, seed=7)
    for _ in range(2):
        tr.train_step(batch)
    a = tr.optimizer.state_dict()
    assert a['acc.emb.seq_item'].shape == (cfg.seq_item_vocab, cfg.seq_feature_dim)
    assert (a['acc.emb.seq_item'] != np.float32(cfg.adagrad_initial_accumulator)).any()
    _, tr2 = _trainer(dev, **adam)
    bad = dict(a)
    bad['acc.emb.seq_item'] = a['acc.emb.seq_item'][:-1]
    with pytest.raises(ValueError, match='acc.emb.seq_item'):
        tr2.optimizer.load_state_dict(bad)
    assert tr2.optimizer.steps_done == 0 and not tr2.optimizer.m.any()
    tr2.optimizer.load_state_dict(a)
    b = tr2.optimizer.state_dict()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    n = st.local_rows
    assert torch.equal(tr2.optimizer.acc['emb.seq_item'][:n], tr.optimizer.acc['emb.seq_item'][:n])
