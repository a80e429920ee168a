"""GPU: the weighted, partially labelled multi-task loss and metrics against the float64 references
of tests/weighted_ref.py: the loss kernels, zero-weight selection, the equivalences with the un-weighted kernels, the
weighted metric state, the model-level loss and gradients, and the trainer / evaluator.

Bounds.  Loss kernels: those of tests/test_glue_kernels_gpu.py::test_task_loss_logits scaled by the new factors:
loss rtol 1e-5; gradient rtol 1e-5 plus atol 2^-24 gscale a_t w / denom_t (the f32 rounding of p), 2.5 times that
for an MSE task.  Metrics: the integer state exactly, the double sums rtol 1e-12.  Model level: those of
tests/test_model_gpu.py (loss 1e-4, gradients 2e-4 of the gradient's largest element); twice that between two GPU
runs, each within one bound of the oracle."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd.data import gate_task_weights, make_batch, make_request_batch
from recommend_amd.evaluate import OneTransEvaluator
from recommend_amd.metrics import StreamingMetrics
from recommend_amd.model import OneTransModel, keras_bce_loss
from recommend_amd.params import init_params
from recommend_amd.trainer import OneTransTrainer, stack_labels, stack_weights

import streaming_metrics_ref as SR
import weighted_ref as WR
from test_request_train_gpu import GRAD_TOL, close, grads_of, small, t_

SENT = -77.0
Z_EDGES = [(40.0, 0.0), (40.0, 1.0), (-40.0, 0.0), (-40.0, 1.0), (100.0, 0.0), (100.0, 1.0), (-100.0, 0.0),
           (-100.0, 1.0)]
P_EDGES = [(0.0, 0.0), (0.0, 1.0), (1.0, 1.0)]
W_VALUES = np.float32([0.0, 0.25, 1.0, 1.0, 2.5, 1.0 / 0.3, 40.0])
SCALE = [0.5, 2.0, 1.25]


# ---- 1. the loss kernels ----------------------------------------------------------------------------------------

def loss_inputs(T, B, mse_mask, prob_form, seed):
    """(z, p, y, w [T, B]) float32: logits N(0, 2) with the +-40 / +-100 edges (probability form: U(0.001, 0.999)
    with p = 0 / 1 edges), labels 0/1 (BCE) or U(0, 1) (MSE), weights from W_VALUES (zeros included) and
    U(0, 3); at least one positive weight per task."""
    rng = np.random.default_rng(seed)
    mse = np.array([(mse_mask >> t) & 1 for t in range(T)], bool)
    y = (rng.random((T, B)) < 0.3).astype(np.float32)
    y[mse] = rng.random((int(mse.sum()), B)).astype(np.float32)
    if prob_form:
        p = rng.uniform(0.001, 0.999, (T, B)).astype(np.float32)
        z = np.zeros((T, B), np.float32)
        edges, v = P_EDGES, p
    else:
        z = rng.normal(0.0, 2.0, (T, B)).astype(np.float32)
        edges, v = Z_EDGES, z
    if B >= 5:
        for t in range(T):
            for j in range(min(B - 1, len(edges))):
                v[t, j], yy = edges[(j + t) % len(edges)]
                if not mse[t]:
                    y[t, j] = yy
    if not prob_form:
        p = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    w = np.where(rng.random((T, B)) < 0.5, rng.choice(W_VALUES, (T, B)), rng.uniform(0.0, 3.0, (T, B))).astype(np.float32)
    w[:, -1] = 1.5
    return z, p, y, w


def run_loss(dev, z, p, y, w, wstride, scale, mse_mask, reduction, prob_form, gscale):
    """One forward and backward through the kernels; every output has a sentinel behind it."""
    T, B = y.shape
    z_d = None if prob_form else torch.from_numpy(z).to(dev)
    p_d, y_d = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    w_d = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    s_d = None if scale is None else torch.tensor(scale, dtype=torch.float32, device=dev)
    loss = torch.full((2,), SENT, device=dev)
    denom = torch.full((T + 1,), SENT, device=dev)
    K.task_loss_weighted_fwd(z_d, p_d, y_d, w_d, wstride, s_d, T, B, loss, denom, device=dev, mse_mask=mse_mask,
                             reduction=reduction)
    dout = torch.full((T * B + 1,), SENT, device=dev)
    K.task_loss_weighted_bwd(p_d, y_d, w_d, wstride, s_d, denom, torch.tensor([gscale], device=dev), T, B, dout,
                             mse_mask=mse_mask, prob_form=prob_form)
    loss, denom, dout = loss.cpu().numpy(), denom.cpu().numpy(), dout.cpu().numpy()
    assert loss[1] == SENT and denom[T] == SENT and dout[-1] == SENT
    return loss[0], denom[:T], dout[:-1].reshape(T, B)


def bits(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float32)).view(np.uint32).tobytes()


def check_loss(got, ref, T, mse_mask, scale, gscale):
    loss, denom, g = got
    rloss, rg, rden, wc = ref
    assert np.isfinite(loss) and np.isfinite(g).all()
    np.testing.assert_allclose(loss, rloss, rtol=1e-5)
    np.testing.assert_allclose(denom, rden, rtol=1e-6)
    a = np.ones(T) if scale is None else np.asarray(scale, np.float64)
    k = np.array([2.5 if (mse_mask >> t) & 1 else 1.0 for t in range(T)])
    atol = 2.0 ** -24 * gscale * (a * k)[:, None] * wc / np.where(rden > 0, rden, 1.0)[:, None]
    err = np.abs(g - rg)
    bad = err > atol + 1e-5 * np.abs(rg)
    assert not bad.any(), (int(bad.sum()), float(err.max()))


@pytest.mark.parametrize('reduction', ['batch', 'weights'])
@pytest.mark.parametrize('prob_form', [False, True], ids=['logits', 'probs'])
@pytest.mark.parametrize('B', [1, 5, 256, 257, 65537])
@pytest.mark.parametrize('T', [1, 3])
def test_loss_kernels_match_float64(dev, T, B, prob_form, reduction):
    """B: one thread, a partial block, an exact block, one over, more than the 256 grid-strided blocks.  Every case
    runs an mse_mask with a set bit, a task_scale, and per-task ([T, B], stride B) and shared ([B], stride 0)
    weights; logits of +-40 and +-100 stay finite."""
    gscale = 1.7
    for mse_mask in ((0, 1) if T == 1 else (0b010,)):
        z, p, y, w = loss_inputs(T, B, mse_mask, prob_form, seed=1000 * T + B + 7 * mse_mask)
        for wstride, scale in ((B, SCALE[:T]), (0, None), (0, SCALE[:T])):
            wk = w if wstride else w[0]
            ref = WR.kernel_ref(z, p, y, np.broadcast_to(wk, (T, B)), mse_mask, scale, reduction, prob_form, gscale)
            got = run_loss(dev, z, p, y, wk, wstride, scale, mse_mask, reduction, prob_form, gscale)
            check_loss(got, ref, T, mse_mask, scale, gscale)


# ---- 2. zero-weight selection -------------------------------------------------------------------------------------

@pytest.mark.parametrize('reduction', ['batch', 'weights'])
@pytest.mark.parametrize('prob_form', [False, True], ids=['logits', 'probs'])
def test_zero_weight_selects_the_entry_out(dev, prob_form, reduction):
    T, B, mse_mask, gscale = 3, 257, 0b100, 0.9
    z, p, y, w = loss_inputs(T, B, mse_mask, prob_form, seed=11)
    w[1] = 0.0                                                   # a task without any weight
    dead = w == 0
    assert dead[0].any() and dead[2].any() and not dead[0].all()
    zb, pb, yb = z.copy(), p.copy(), y.copy()
    rng = np.random.default_rng(12)
    zb[dead] = rng.choice(np.float32([np.inf, -np.inf, np.nan]), int(dead.sum()))
    pb[dead] = rng.choice(np.float32([np.nan, np.inf, -1.0]), int(dead.sum()))
    yb[dead] = np.nan
    clean = run_loss(dev, z, p, y, w, B, SCALE, mse_mask, reduction, prob_form, gscale)
    dirty = run_loss(dev, zb, pb, yb, w, B, SCALE, mse_mask, reduction, prob_form, gscale)
    again = run_loss(dev, zb, pb, yb, w, B, SCALE, mse_mask, reduction, prob_form, gscale)
    for a, b in ((clean, dirty), (dirty, again)):                # bit for bit: the loss, the denominators, the gradient
        assert all(bits(x) == bits(v) for x, v in zip(a, b))
    loss, denom, g = dirty
    assert np.isfinite(loss) and np.isfinite(g).all()
    assert np.all(g[dead] == 0.0)
    live = ~dead[[0, 2]]
    assert np.count_nonzero(g[[0, 2]][live]) > 0.9 * live.sum()
    if reduction == 'weights':                                   # the empty task: loss 0, gradient 0, no NaN
        assert denom[1] == 0.0 and np.all(g[1] == 0.0)
        only = run_loss(dev, zb[1:2], pb[1:2], yb[1:2], w[1:2], B, None, 0, reduction, prob_form, gscale)
        assert only[0] == 0.0 and np.all(only[2] == 0.0)
    else:
        assert denom[1] == B and np.all(g[1] == 0.0)


def test_device_weights_are_clamped_not_read_back(dev):
    """A device tensor holding NaN, -1 and 1e9 behaves as 0, 0 and 65536."""
    T, B, gscale = 2, 64, 1.0
    z, p, y, w = loss_inputs(T, B, 0, False, seed=21)
    raw, eff = w.copy(), w.copy()
    raw[:, 20], raw[:, 21], raw[:, 22] = np.nan, -1.0, 1e9      # (ordinary logits: the edges sit in columns 0..7)
    eff[:, 20], eff[:, 21], eff[:, 22] = 0.0, 0.0, 65536.0
    for reduction in ('batch', 'weights'):
        a = run_loss(dev, z, p, y, raw, B, None, 0, reduction, False, gscale)
        b = run_loss(dev, z, p, y, eff, B, None, 0, reduction, False, gscale)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.all(a[2][:, 20:22] == 0.0) and np.all(a[2][:, 22] != 0.0)
    y_d, p_d = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    ma, mb = StreamingMetrics(['ctr', 'cvr'], dev, weighted=True), StreamingMetrics(['ctr', 'cvr'], dev, weighted=True)
    ma.update(y_d, p_d, weights=torch.from_numpy(raw).to(dev))
    mb.update(y_d, p_d, weights=torch.from_numpy(eff).to(dev))
    assert torch.equal(ma._state, mb._state)
    assert int(ma.counts[0].sum()) == int(WR.units(eff[0]).sum())


# ---- 3. equivalences with the un-weighted kernels -----------------------------------------------------------------

@pytest.mark.parametrize('B', [5, 257, 65537])
def test_equivalence_with_the_unweighted_kernels(dev, B):
    T, mse_mask, gscale = 3, 0b010, 1.7
    z, p, y, _ = loss_inputs(T, B, mse_mask, False, seed=31 + B)

    def existing(z, p, y):
        Tn, Bn = y.shape
        z_d, p_d, y_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (z, p, y))
        loss = torch.empty(1, device=dev)
        K.task_loss_logits_fwd(z_d, p_d, y_d, Tn, Bn, loss, device=dev, mse_mask=mse_mask)
        d = torch.empty(Tn, Bn, device=dev)
        K.task_loss_logits_bwd(p_d, y_d, torch.tensor([gscale], device=dev), Tn, Bn, d, mse_mask=mse_mask)
        return loss.item(), d.cpu().numpy().astype(np.float64)

    k = np.array([2.5 if (mse_mask >> t) & 1 else 1.0 for t in range(T)])[:, None]
    # all-ones weights under 'batch'
    ones = np.ones(B, np.float32)
    loss, denom, g = run_loss(dev, z, p, y, ones, 0, None, mse_mask, 'batch', False, gscale)
    rl, rg = existing(z, p, y)
    np.testing.assert_allclose(loss, rl, rtol=1e-5)
    assert np.all(np.abs(g - rg) <= 2.0 ** -24 * gscale * k / B + 1e-5 * np.abs(rg))
    # 0/1 weights under 'weights': the existing kernel on the kept subset
    keep = np.random.default_rng(B).random(B) < 0.6
    keep[-1] = True
    loss, denom, g = run_loss(dev, z, p, y, keep.astype(np.float32), 0, None, mse_mask, 'weights', False, gscale)
    rl, rg = existing(z[:, keep], p[:, keep], y[:, keep])
    n = int(keep.sum())
    assert np.all(denom == n)
    np.testing.assert_allclose(loss, rl, rtol=1e-5)
    assert np.all(g[:, ~keep] == 0.0)
    assert np.all(np.abs(g[:, keep] - rg) <= 2.0 ** -24 * gscale * k / n + 1e-5 * np.abs(rg))


# ---- 4. the weighted metric state ---------------------------------------------------------------------------------

def metric_inputs(B, seed):
    """[3, B] labels, probabilities, weights: task 0 binary; weights from W_VALUES, U(0, 3) (not multiples of 2^-24)
    and a few above the range; a NaN probability under a zero weight (task 0) and under a positive one (task 2)."""
    y, p = SR.make_inputs(3, B, seed)
    rng = np.random.default_rng(seed + 1)
    w = np.where(rng.random((3, B)) < 0.5, rng.choice(W_VALUES, (3, B)), rng.uniform(0.0, 3.0, (3, B))).astype(np.float32)
    w[:, -1] = 1.5
    if B >= 5:
        w[1, 1] = 1e6                                            # clamped to 65536
        w[0, 2], p[0, 2], y[0, 2] = 0.0, np.nan, np.nan         # skipped whatever it holds
        w[2, 3], p[2, 3] = 2.0, np.nan                           # counted: bin 0, NaN sums
    return y, p, w


def run_metrics(dev, m, y, p, w, off, shared=False):
    """One ot_metrics_update_weighted call into fresh state; the three operands start ``off`` floats past a 16-byte
    boundary (off 1: the scalar path) with a row stride that is a multiple of 4."""
    T, B = y.shape
    stride = (B + 3) // 4 * 4

    def place(a):
        buf = torch.full((T * stride + 8,), float('nan'), device=dev)
        view = buf[off:off + T * stride].view(T, stride)
        view[:, :B] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        assert (view.data_ptr() % 16 == 0) == (off % 4 == 0)
        return buf, view
    (by, vy), (bp, vp), (bw, vw) = place(y), place(p), place(w)
    state = torch.zeros_like(m._state)
    nc = m.counts.numel()
    counts, sums = state[:nc], state[nc:].view(torch.float64)
    K.metrics_update_weighted(vp, vy, vw[0] if shared else vw, T, B, stride, 0 if shared else stride, m.bounds, m.nb,
                              counts, sums, device=dev)
    return state, counts.view(m.counts.shape).cpu().numpy(), sums.view(T, 4).cpu().numpy()


@pytest.mark.parametrize('B', [1, 5, 1024, 1027, 131077])
def test_weighted_metric_state_matches_numpy(dev, B):
    """B: a quad tail, one workgroup pass, one over, past 128 workgroups x 1024 samples.  The integer state is exact,
    the double sums within rtol 1e-12; the vector and the scalar path and two runs give the same bits."""
    m = StreamingMetrics(['ctr', 'cvr', 'watch'], dev, weighted=True)
    y, p, w = metric_inputs(B, seed=40 + B)
    rc, rs = WR.ref_state_weighted(y, p, w, m.bounds_host)
    states = []
    for off in (0, 1, 0):
        state, counts, sums = run_metrics(dev, m, y, p, w, off)
        states.append(state)
        assert np.array_equal(counts, rc)
        assert np.array_equal(sums[:, 0], rs[:, 0])
        assert np.array_equal(np.isnan(sums), np.isnan(rs)) and (B < 5 or np.isnan(sums[2, 1:]).all())
        ok = ~np.isnan(rs)
        assert SR.rel_close(sums[ok], rs[ok], 1e-12)
    assert torch.equal(states[0], states[1]) and torch.equal(states[0], states[2])
    # one [B] row for every task (weight stride 0)
    rc, rs = WR.ref_state_weighted(y, p, w[0], m.bounds_host)
    _, counts, sums = run_metrics(dev, m, y, p, w, 1, shared=True)
    ok = ~np.isnan(rs)
    assert np.array_equal(counts, rc) and np.array_equal(sums[:, 0], rs[:, 0]) and SR.rel_close(sums[ok], rs[ok], 1e-12)


def test_integer_weights_equal_replicated_records(dev):
    """Weights k in {0..3}: the state is OT_METRICS_WEIGHT_ONE times the un-weighted kernel's on the k-fold replicated
    records (counts exactly, sums rtol 1e-12); an update without weights on a weighted object counts every sample
    once."""
    B = 1027
    tasks = ['ctr', 'cvr', 'watch']
    y, p = SR.make_inputs(3, B, seed=51)
    p[2, 7] = np.nan
    k = np.random.default_rng(52).integers(0, 4, B)
    k[7] = 2
    y_d, p_d = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    mw, mu = StreamingMetrics(tasks, dev, weighted=True), StreamingMetrics(tasks, dev)
    mw.update(y_d, p_d, weights=torch.from_numpy(k.astype(np.float32)).to(dev))
    mu.update(torch.from_numpy(np.repeat(y, k, axis=1)).to(dev), torch.from_numpy(np.repeat(p, k, axis=1)).to(dev))
    one = StreamingMetrics.WEIGHT_ONE
    assert torch.equal(mw.counts, mu.counts * one)
    sw, su = mw.sums.cpu().numpy(), mu.sums.cpu().numpy() * one
    assert np.array_equal(sw[:, 0], su[:, 0]) and np.array_equal(np.isnan(sw), np.isnan(su)) and np.isnan(sw[2, 1])
    assert SR.rel_close(sw[~np.isnan(su)], su[~np.isnan(su)], 1e-12)
    mw.reset_states()
    mu.reset_states()
    mw.update(y_d, p_d)
    mu.update(y_d, p_d)
    assert torch.equal(mw.counts, mu.counts * one)
    sw, su = mw.sums.cpu().numpy(), mu.sums.cpu().numpy() * one
    assert np.array_equal(sw[:2], su[:2]) and np.array_equal(sw[2, 0], su[2, 0])     # same walk, exact scaling by 2^24


def test_zero_one_weights_report_the_kept_subset(dev):
    B = 1500
    tasks = ['ctr', 'cvr', 'watch']
    y, p = SR.make_inputs(3, B, seed=61)
    y[1] = (y[1] > 0.5).astype(np.float32)
    keep = np.random.default_rng(62).random(B) < 0.4
    yb = y.copy()
    yb[:, ~keep] = np.nan                                        # unlabelled where the weight is 0
    mw, mu = StreamingMetrics(tasks, dev, weighted=True), StreamingMetrics(tasks, dev)
    mw.update(torch.from_numpy(yb).to(dev), torch.from_numpy(p).to(dev),
              weights=torch.from_numpy(keep.astype(np.float32)).to(dev))
    mu.update(torch.from_numpy(y[:, keep]).to(dev), torch.from_numpy(p[:, keep]).to(dev))
    rw, ru = mw.result(extended=True), mu.result(extended=True)
    assert set(rw) == set(ru)
    for key, v in ru.items():
        if key.rsplit('_', 1)[1] in ('mse', 'mae', 'logloss'):
            assert rw[key] == pytest.approx(v, rel=1e-12), key
        else:
            assert rw[key] == v, key                             # from integer counts scaled by 2^24: exact


# ---- 5. model level -----------------------------------------------------------------------------------------------

TASK_W = {'ctr': 1.0, 'cvr': 0.5}


def weighted_batch(cfg, B=7, seed=1000):
    """``make_batch`` with sample weights and a CVR weight gated on the click; CVR labels are NaN without a click."""
    ns, seq, lab = make_batch(B, cfg, seed=seed)
    lab = gate_task_weights(lab)
    assert 0 < lab['cvr_weight'].sum() < B
    lab['cvr'] = np.where(lab['cvr_weight'] > 0, lab['cvr'], np.float32(np.nan)).astype(np.float32)
    lab['sample_weight'] = np.float32([1.0, 2.5, 0.5, 1.0, 4.0, 1.0, 0.25] * B)[:B].reshape(B, 1)
    return ns, seq, lab


def cat_batches(a, b):
    """Two batches (3-tuples, or request-grouped 4-tuples) as one: b's rows after a's."""
    cat = lambda x, y: {k: np.concatenate([x[k], y[k]]) for k in x}
    out = (cat(a[0], b[0]), cat(a[1], b[1]), cat(a[2], b[2]))
    if len(a) == 4:
        out += (np.concatenate([a[3], b[3] + a[1][next(iter(a[1]))].shape[0]]).astype(np.int32),)
    return out


def zero_weighted(cfg, X, Z):
    """X with Z appended under sample weight 0 and NaN labels."""
    nz = len(Z[2][cfg.tasks[0]])
    nx = len(X[2][cfg.tasks[0]])
    zl = {t: np.full_like(Z[2][t], np.nan) for t in cfg.tasks}
    xl = {t: X[2][t] for t in cfg.tasks}
    both = cat_batches(X[:2] + (xl,) + X[3:], Z[:2] + (zl,) + Z[3:])
    both[2]['sample_weight'] = np.concatenate([np.ones((nx, 1), np.float32), np.zeros((nz, 1), np.float32)])
    return both


def run_model(model, cfg, batch, dev, weighted):
    """Forward, loss and backward through the model (no optimizer step): (loss, dense grads, sparse grads)."""
    ns, seq, lab = batch[:3]
    model.flat.grad.fill_(float('nan'))
    model._pending_sparse = []
    if len(batch) == 4:
        probs = model.forward_probs_requests(t_(ns, dev), t_(seq, dev), torch.from_numpy(batch[3]).to(dev), training=False)
    else:
        probs = model.forward_probs(t_(ns, dev), t_(seq, dev), training=False)
    y = stack_labels(lab, cfg.tasks, dev)
    if weighted:
        w = stack_weights(lab, cfg, dev)
        scale = [cfg.task_loss_weights.get(t, 1.0) for t in cfg.tasks]
        loss = keras_bce_loss(y, probs, cfg.tasks, 2, weights=w, task_scale=scale, reduction=cfg.loss_reduction)
    else:
        loss = keras_bce_loss(y, probs, cfg.tasks, 2)
    loss.backward()
    g, sp = grads_of(model)
    return loss.item(), g, sp


def compare_grads(got, want, mult, what, oracle=False):
    (gd, gs), (wd, ws) = got, want
    for name, g in gd.items():
        r = wd[name]
        if oracle and name == 'tok.ns.kernel':                   # the model pads the kernel's rows
            assert torch.all(g[r.shape[0]:] == 0)
            g = g[:r.shape[0]]
        close(g, r, mult * GRAD_TOL, f'{what} {name}')
    assert set(gs) == {'emb.ns', 'emb.seq_item'}
    for name in gs:
        close(gs[name], ws[name], mult * GRAD_TOL, f'{what} {name}')


@pytest.mark.parametrize('reduction', ['batch', 'weights'])
def test_model_loss_and_gradients_match_the_oracle(dev, reduction):
    cfg = small()
    cfg.weighted_loss, cfg.loss_reduction, cfg.task_loss_weights = True, reduction, dict(TASK_W)
    batch = weighted_batch(cfg)
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=dev, init=P)
    loss, g, sp = run_model(model, cfg, batch, dev, weighted=True)
    w = stack_weights(batch[2], cfg, 'cpu').numpy()
    rl, rg, _ = WR.model_loss_and_grads(P, cfg, batch[0], batch[1], batch[2], w,
                                        scale=[TASK_W[t] for t in cfg.tasks], reduction=reduction)
    print(f'{reduction}: loss {loss:.6f} vs {rl:.6f}')
    assert abs(loss - rl) < 1e-4
    dense = {k: v for k, v in rg.items() if not k.startswith('emb.')}
    sparse = {k: v for k, v in rg.items() if k.startswith('emb.')}
    compare_grads((g, sp), (dense, sparse), 1, reduction, oracle=True)


def z_only_rows(X, Z):
    """Rows of the item table that only Z's sequences reference."""
    ids = lambda b: set(np.concatenate([np.asarray(v).reshape(-1) for v in b[1].values()]).tolist())
    rows = sorted(ids(Z) - ids(X))
    assert rows
    return torch.tensor(rows)


@pytest.mark.parametrize('grouped', [False, True], ids=['samples', 'requests'])
def test_zero_weight_samples_leave_no_trace(dev, grouped):
    """X with zero-weight, unlabelled samples Z appended, under 'weights', against X alone with the switch off: the
    loss and every gradient within twice the oracle bounds; after a train_step the item-table rows that only Z
    references keep weight and Adagrad accumulator bit for bit, and no table row changes that X alone leaves alone."""
    cfg = small()
    if grouped:
        X = make_request_batch(3, [3, 0, 4], cfg, seed=1000)
        Z = make_request_batch(2, [2, 2], cfg, seed=2000)
    else:
        X, Z = make_batch(7, cfg, seed=1000), make_batch(4, cfg, seed=2000)
    XZ = zero_weighted(cfg, X, Z)
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    on = small()
    on.weighted_loss, on.loss_reduction = True, 'weights'
    m_off, m_on = OneTransModel(cfg, device=dev, init=P), OneTransModel(on, device=dev, init=P)
    l_off, g_off, s_off = run_model(m_off, cfg, X, dev, weighted=False)
    l_on, g_on, s_on = run_model(m_on, on, XZ, dev, weighted=True)
    print(f'loss {l_on:.6f} vs {l_off:.6f}')
    assert abs(l_on - l_off) < 2e-4
    compare_grads((g_on, s_on), (g_off, s_off), 2, 'XZ vs X')
    rows = z_only_rows(X, Z)
    assert torch.all(s_on['emb.seq_item'][rows] == 0)

    t_off, t_on = OneTransTrainer(cfg, model=m_off), OneTransTrainer(on, model=m_on)
    before = {k: (v.clone(), t_on.optimizer.acc[k].clone()) for k, v in m_on.tables.items()}
    m_off._pending_sparse, m_on._pending_sparse = [], []         # (the gradients taken above are not applied)
    out_off, out_on = t_off.train_step(X), t_on.train_step(XZ)
    assert abs(out_on['total_loss'].item() - out_off['total_loss'].item()) < 2e-4
    tab, acc = m_on.tables['emb.seq_item'], t_on.optimizer.acc['emb.seq_item']
    r = rows.to(dev)
    assert torch.equal(tab[r], before['emb.seq_item'][0][r]) and torch.equal(acc[r], before['emb.seq_item'][1][r])
    for k, (w0, a0) in before.items():
        changed_on = ((m_on.tables[k] != w0) | (t_on.optimizer.acc[k] != a0)).any(dim=1)
        init_acc = torch.full_like(a0, float(cfg.adagrad_initial_accumulator))
        changed_off = ((m_off.tables[k] != w0) | (t_off.optimizer.acc[k] != init_acc)).any(dim=1)
        assert changed_off.any() and not (changed_on & ~changed_off).any(), k


@pytest.mark.parametrize('rank', [2, 1])
def test_switch_off_ignores_weight_keys(dev, rank):
    """With config.weighted_loss off the weight keys are inert: a train_step and a val_step give the same bits as
    without them — also with [B] labels (the probability-form BCE) beside [B, 1] weight arrays."""
    cfg = small()
    ns, seq, lab = make_batch(7, cfg, seed=1000)
    if rank == 1:
        lab = {t: v.reshape(-1) for t, v in lab.items()}
    extra = dict(lab, sample_weight=np.full((7, 1), 3.0, np.float32), cvr_weight=np.zeros((7, 1), np.float32))
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    outs = []
    for labels in (lab, extra):
        tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, init=P))
        tr.enable_metrics()
        step = tr.train_step((ns, seq, labels))
        val = tr.val_step((ns, seq, labels))
        outs.append((step['total_loss'], step['probs'], val['total_loss'], val['probs'], tr.model.flat.data.clone(),
                     tr.train_metrics._state.clone(), tr.val_metrics._state.clone())
                    + tuple(t.clone() for t in tr.model.tables.values()))
        assert not tr.train_metrics.weighted
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 6. trainer and evaluator ---------------------------------------------------------------------------------------

def want_metrics(cfg, m, lab, probs, extended):
    w = stack_weights(lab, cfg, 'cpu').numpy()
    y = stack_labels(lab, cfg.tasks, 'cpu').numpy()
    p = probs.cpu().numpy()
    names = ('auc', 'accuracy', 'precision', 'recall') + (('f1', 'logloss') if extended else ())
    out = {}
    for i, t in enumerate(cfg.tasks):
        r = WR.weighted_metrics(y[i], p[i], w[i], m.thresholds)
        out.update({f'{t}_{k}': r[k] for k in names})
    return out


def test_trainer_and_evaluator_report_weighted_metrics(dev):
    cfg = small()
    cfg.weighted_loss, cfg.loss_reduction, cfg.task_loss_weights = True, 'weights', dict(TASK_W)
    batch = weighted_batch(cfg, B=48)
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, init=P))
    tr.enable_metrics()
    assert tr.train_metrics.weighted and tr.val_metrics.weighted
    val = tr.val_step(batch)
    got = tr.metric_results(tr.val_metrics)
    want = want_metrics(cfg, tr.val_metrics, batch[2], val['probs'], extended=False)
    assert set(got) == set(want)
    assert all(got[k] == pytest.approx(v, rel=1e-10, abs=1e-12) for k, v in want.items()), (got, want)
    step = tr.train_step(batch)
    got = tr.metric_results(tr.train_metrics)
    want = want_metrics(cfg, tr.train_metrics, batch[2], step['probs'], extended=False)
    assert all(got[k] == pytest.approx(v, rel=1e-10, abs=1e-12) for k, v in want.items()), (got, want)
    assert torch.isfinite(step['total_loss']) and torch.isfinite(val['total_loss'])

    # the offline evaluator reads the same keys (after the step: new weights, new probabilities)
    ev = OneTransEvaluator(tr.model, cfg)
    res = ev.evaluate_offline([batch])
    probs = tr.val_step(batch)['probs']
    want = want_metrics(cfg, ev.metrics, batch[2], probs, extended=True)
    assert all(res[k] == pytest.approx(v, rel=1e-10, abs=1e-12) for k, v in want.items()), (res, want)
    unweighted = StreamingMetrics(cfg.tasks, dev)
    y = stack_labels({t: np.nan_to_num(batch[2][t]) for t in cfg.tasks}, cfg.tasks, dev)
    unweighted.update(y, probs)
    assert abs(unweighted.result()['ctr_auc'] - res['ctr_auc']) > 1e-6       # the weights do change the report

    # host-side evaluate(): the weighted rank AUC
    w = stack_weights(batch[2], cfg, 'cpu').numpy()
    host = tr.evaluate([batch])
    from recommend_amd.metrics import auc
    yy = stack_labels(batch[2], cfg.tasks, 'cpu').numpy()
    for i, t in enumerate(cfg.tasks):
        assert host[f'{t}_auc'] == auc(yy[i], probs.cpu().numpy()[i], weights=w[i])


def test_group_feature_with_weights_is_refused(dev):
    cfg = small()
    cfg.weighted_loss = True
    feature = list(cfg.sparse_features)[0]
    batch = weighted_batch(cfg)
    plain = (batch[0], batch[1], {t: np.nan_to_num(batch[2][t]) for t in cfg.tasks})
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    tr = OneTransTrainer(cfg, model=OneTransModel(cfg, device=dev, init=P))
    tr.enable_metrics(group_feature=feature)
    with pytest.raises(NotImplementedError, match='grouped AUC'):
        tr.train_step(batch)
    with pytest.raises(NotImplementedError, match='grouped AUC'):
        tr.val_step(batch)
    with pytest.raises(NotImplementedError, match='grouped AUC'):
        OneTransEvaluator(tr.model, cfg, group_feature=feature).evaluate_offline([batch])
    tr.train_step(plain)                                         # no weight key in the batch: as before
    tr.val_step(plain)
    res = tr.metric_results(tr.val_metrics)
    assert 'ctr_uauc' in res and np.isfinite(res['ctr_auc'])
    assert tr.val_grouped.count == 7 and tr.train_grouped.count == 7
