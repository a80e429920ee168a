"""The model-glue kernels (model_io.hip, ot_rows_colsum) called directly through the C ABI, each against a float64
torch / numpy reference of the same operation, at the sizes where they take another branch than in the whole-model
tests: more samples than the head backward's grid covers in one pass, more loss elements than the loss grid, more
partial rows than the one-level column reduce."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd._lib import NS_FIELD_BYTES, OneTransHipError, call, size
from oracle import keras_math as km

TOL = dict(rtol=2e-5, atol=2e-5)          # test_kernels_gpu.TOL
SUM_TOL = dict(rtol=1e-4, atol=1e-4)      # sums over the batch (dw2, db2)
SENT = -77.0


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---- task heads -----------------------------------------------------------------------------------------------

def _head_ref(pre1, w2, b2, T, B, dh, dprobs, dlogits):
    """z[t][b] = gelu(pre1[t B + b]) . w2[t] + b2[t], p = sigmoid(z) in float64; the gradients of
    sum(p dprobs) + sum(z dlogits) by autograd."""
    x = pre1.clone().requires_grad_(True)
    w = w2.clone().requires_grad_(True)
    b = b2.clone().requires_grad_(True)
    z = (gelu64(x).view(T, B, dh) * w[:, None, :]).sum(-1) + b[:, None]
    p = torch.sigmoid(z)
    loss = torch.zeros((), dtype=torch.float64)
    if dprobs is not None:
        loss = loss + (p * dprobs.view(T, B)).sum()
    if dlogits is not None:
        loss = loss + (z * dlogits.view(T, B)).sum()
    loss.backward()
    return z.detach().reshape(-1), p.detach().reshape(-1), x.grad, w.grad, b.grad


@pytest.mark.parametrize('dh', [1, 63, 64, 65, 256])
@pytest.mark.parametrize('B', [1, 5, 261])
@pytest.mark.parametrize('T', [1, 3])
def test_head_fwd_bwd(dev, T, B, dh):
    """ot_head_fwd, ot_head_bwd (dprobs) and ot_head_bwd_ex (dlogits alone, then both) vs float64 autograd.  B = 261:
    the backward's 64 blocks of 4 samples take a second, ragged pass.  dw2 / db2 are written with task strides larger
    than dh / 1 (the gaps keep their sentinel) and, with accumulate, added onto what is there."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + dh)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    pre1, w2, b2 = rnd(T * B, dh), rnd(T, dh) / math.sqrt(dh), 0.3 * rnd(T)
    dprobs, dlogits = rnd(T * B), rnd(T * B)
    f = lambda x: x.float().to(dev).contiguous()
    pre1_d, w2_d, b2_d, dp_d, dl_d = f(pre1), f(w2), f(b2), f(dprobs), f(dlogits)
    pre1, w2, b2, dprobs, dlogits = (x.double().cpu() for x in (pre1_d, w2_d, b2_d, dp_d, dl_d))   # the f32 values

    logits = torch.full((T * B + 1,), SENT, device=dev)
    probs = torch.full((T * B + 1,), SENT, device=dev)
    K.head_fwd(pre1_d, w2_d, b2_d, T, B, dh, logits, probs)
    z_ref, p_ref, _, _, _ = _head_ref(pre1, w2, b2, T, B, dh, None, dlogits)
    assert logits[-1].item() == SENT and probs[-1].item() == SENT
    torch.testing.assert_close(logits[:-1].double().cpu(), z_ref, **TOL)
    torch.testing.assert_close(probs[:-1].double().cpu(), p_ref, **TOL)
    probs_d = probs[:-1].contiguous()

    sw2, sb2 = dh + 3, 2
    base_w = torch.randn(T, sw2, dtype=torch.float64, generator=g).float()
    base_b = torch.randn(T, sb2, dtype=torch.float64, generator=g).float()
    ws = K.workspace(size('ot_head_bwd_workspace_size', T, B, dh), dev)
    for use_p, use_l, accumulate in [(True, False, False), (False, True, False), (True, True, False),
                                     (True, True, True), (True, False, True)]:
        _, _, dx_ref, dw_ref, db_ref = _head_ref(pre1, w2, b2, T, B, dh, dprobs if use_p else None,
                                                 dlogits if use_l else None)
        dpre1 = torch.full((T * B + 1, dh), SENT, device=dev)
        dw2, db2 = base_w.to(dev), base_b.to(dev)
        if use_p and not use_l:              # the plain entry point
            call('ot_head_bwd', K.ptr(pre1_d), K.ptr(w2_d), K.ptr(probs_d), K.ptr(dp_d), T, B, dh, K.ptr(dpre1),
                 K.ptr(dw2), K.ptr(db2), sw2, sb2, int(accumulate), K.ptr(ws), ws.numel(), K.stream())
        else:
            K.head_bwd(pre1_d, w2_d, probs_d, dp_d if use_p else None, T, B, dh, dpre1, dw2, db2, sw2, sb2,
                       accumulate=accumulate, device=dev, dlogits=dl_d if use_l else None)
        assert bool((dpre1[-1] == SENT).all())
        torch.testing.assert_close(dpre1[:-1].double().cpu(), dx_ref, **TOL)
        dw2, db2 = dw2.cpu(), db2.cpu()
        assert torch.equal(dw2[:, dh:], base_w[:, dh:]) and torch.equal(db2[:, 1:], base_b[:, 1:])
        add_w = base_w[:, :dh].double() if accumulate else 0.0
        add_b = base_b[:, 0].double() if accumulate else 0.0
        torch.testing.assert_close(dw2[:, :dh].double(), dw_ref + add_w, **SUM_TOL)
        torch.testing.assert_close(db2[:, 0].double(), db_ref + add_b, **SUM_TOL)


def test_head_bwd_refuses_wide_hidden(dev):
    """dh = 257 > 256: both backward entry points return an error before any launch and write nothing."""
    T, B, dh = 2, 3, 257
    pre1, w2 = torch.randn(T * B, dh, device=dev), torch.randn(T, dh, device=dev)
    probs, dprobs = torch.rand(T * B, device=dev), torch.randn(T * B, device=dev)
    dpre1 = torch.full((T * B, dh), SENT, device=dev)
    dw2, db2 = torch.full((T, dh), SENT, device=dev), torch.full((T,), SENT, device=dev)
    ws = K.workspace(size('ot_head_bwd_workspace_size', T, B, dh), dev)
    with pytest.raises(OneTransHipError, match='dh=257'):
        K.head_bwd(pre1, w2, probs, dprobs, T, B, dh, dpre1, dw2, db2, dh, 1, device=dev)
    with pytest.raises(OneTransHipError, match='dh=257'):
        call('ot_head_bwd', K.ptr(pre1), K.ptr(w2), K.ptr(probs), K.ptr(dprobs), T, B, dh, K.ptr(dpre1), K.ptr(dw2),
             K.ptr(db2), dh, 1, 0, K.ptr(ws), ws.numel(), K.stream())
    torch.cuda.synchronize()
    assert bool((dpre1 == SENT).all()) and bool((dw2 == SENT).all()) and bool((db2 == SENT).all())


# ---- task loss ------------------------------------------------------------------------------------------------

LOSS_SHAPES = [(1, 1), (3, 37), (32, 5), (2, 40000)]      # (2, 40000): T B > 65536, the blocks of the forward loop
MSE_MASKS = [0, 0b101, 1 << 31]                           # bit 31 names a task only at T = 32
P_HI = float(np.float32(1) - np.float32(2.0 ** -24))      # the f32 value above 1 - 1e-7 (and below 1)
# (p, y) at and beyond the clip bounds.  p >= 1 - 1e-7 is paired with y = 1 here: with y = 0 the loss is
# -log(1 - pc + eps) at pc = "1 - eps", a bound float32 rounds to 1 - 2^-23, which no float32 evaluation (Keras's own
# included) can bring within 1e-5 of the float64 km.keras_bce; test_task_loss_upper_clip_edge covers that pairing.
P_EDGES = [(0.0, 0.0), (0.0, 1.0), (5e-8, 0.0), (5e-8, 1.0), (1.0, 1.0), (P_HI, 1.0)]
Z_EDGES = [(40.0, 0.0), (40.0, 1.0), (-40.0, 0.0), (-40.0, 1.0), (100.0, 0.0), (100.0, 1.0), (-100.0, 0.0),
           (-100.0, 1.0)]


def _is_mse(T, mse_mask):
    return np.array([(mse_mask >> t) & 1 for t in range(T)], bool)


def _loss_inputs(T, B, mse_mask, edges, draw):
    """values [T, B] float32 (``draw``: the ordinary ones; ``edges`` cycled through the head of every task once a
    task has room for them next to ordinary values) and labels (0/1 for a BCE task, U(0, 1) for an MSE task)."""
    rng = np.random.default_rng(100 * T + B + (mse_mask & 0xFF))
    v = draw(rng, (T, B)).astype(np.float32)
    y = (rng.random((T, B)) < 0.3).astype(np.float32)
    mse = _is_mse(T, mse_mask)
    y[mse] = rng.random((int(mse.sum()), B)).astype(np.float32)
    if B >= 5:
        for t in range(T):
            for j in range(min(B - 1, len(edges))):
                v[t, j], yy = edges[(j + t) % len(edges)]
                if not mse[t]:
                    y[t, j] = yy
    return v, y, mse


@pytest.mark.parametrize('mse_mask', MSE_MASKS)
@pytest.mark.parametrize('T,B', LOSS_SHAPES)
def test_task_loss_probs(dev, T, B, mse_mask):
    """ot_task_loss_fwd / ot_task_loss_bwd vs km.keras_bce (BCE tasks) plus mean (p - y)^2 (tasks of mse_mask) summed
    over tasks, rtol 1e-5, and vs float64 autograd of the same expressions times gscale.  Probabilities at 0, 1,
    below 1e-7 and above 1 - 1e-7 give a finite loss and a zero gradient."""
    p, y, mse = _loss_inputs(T, B, mse_mask, P_EDGES, lambda rng, s: rng.uniform(0.001, 0.999, s))
    p_d, y_d = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    loss = torch.full((2,), SENT, device=dev)
    K.bce_fwd(p_d, y_d, T, B, loss, device=dev, mse_mask=mse_mask)
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    ref = sum(float(np.mean((p64[t] - y64[t]) ** 2)) if mse[t] else km.keras_bce(y64[t], p64[t]) for t in range(T))
    got = loss.cpu().numpy()
    assert got[1] == SENT and np.isfinite(got[0])
    np.testing.assert_allclose(got[0], ref, rtol=1e-5)

    gscale = 0.37
    pt = torch.from_numpy(p64).requires_grad_(True)
    yt = torch.from_numpy(y64)
    eps = km.KERAS_EPSILON
    pc = torch.clamp(pt, eps, 1.0 - eps)
    bce = -(yt * torch.log(pc + eps) + (1.0 - yt) * torch.log(1.0 - pc + eps))
    per = torch.where(torch.from_numpy(mse)[:, None], (pt - yt) ** 2, bce)
    (per.mean(1).sum() * gscale).backward()
    dprobs = torch.full((T * B + 1,), SENT, device=dev)
    K.bce_bwd(p_d, y_d, torch.tensor([gscale], device=dev), T, B, dprobs, mse_mask=mse_mask)
    got = dprobs.cpu().numpy()
    assert got[-1] == SENT
    got = got[:-1].reshape(T, B)
    clipped = ((p < 1e-7) | (p > 1 - 1e-7)) & ~mse[:, None]
    assert clipped.sum() >= (6 if B >= 7 else 0) and not got[clipped].any() and not pt.grad.numpy()[clipped].any()
    np.testing.assert_allclose(got, pt.grad.numpy(), rtol=1e-5, atol=1e-9)


def test_task_loss_upper_clip_edge(dev):
    """p >= 1 - 1e-7 with label 0.  Keras clips to 1 - epsilon evaluated in float32, which is 1 - 2^-23, so its term
    is -log(2^-23 + 1e-7) = 15.33, not float64's -log(2e-7) = 15.42: the kernel is compared with the float64 value
    of the float32 bound (rtol 1e-5), is within 1 % of km.keras_bce, and its gradient is zero."""
    p = np.array([[1.0, P_HI, 0.5, 0.25]], np.float32)
    y = np.zeros((1, 4), np.float32)
    loss = torch.full((1,), SENT, device=dev)
    K.bce_fwd(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), 1, 4, loss, device=dev)
    eps = km.KERAS_EPSILON
    hi = float(np.float32(1) - np.float32(eps))
    assert hi == 1.0 - 2.0 ** -23
    pc = np.minimum(p.astype(np.float64), hi)
    ref32 = float(np.mean(-np.log(1.0 - pc + eps)))
    np.testing.assert_allclose(loss.item(), ref32, rtol=1e-5)
    np.testing.assert_allclose(loss.item(), km.keras_bce(y.astype(np.float64), p.astype(np.float64)), rtol=1e-2)
    dprobs = torch.full((4,), SENT, device=dev)
    K.bce_bwd(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), torch.ones(1, device=dev), 1, 4, dprobs)
    got = dprobs.cpu().numpy()
    assert got[0] == 0.0 and got[1] == 0.0
    np.testing.assert_allclose(got[2:], [1 / (0.5 + eps) / 4, 1 / (0.75 + eps) / 4], rtol=1e-5)


@pytest.mark.parametrize('mse_mask', MSE_MASKS)
@pytest.mark.parametrize('T,B', LOSS_SHAPES)
def test_task_loss_logits(dev, T, B, mse_mask):
    """ot_task_loss_logits_fwd / _bwd vs km.keras_bce_logits (BCE tasks, from z) plus mean (p - y)^2 (tasks of
    mse_mask, from p = sigmoid(z)), rtol 1e-5; logits of +-40 and +-100 stay finite.  The backward takes p in
    float32, whose rounding (at most 2^-24 for p < 1) is the gradient's absolute error: atol 2^-24 gscale / B on top
    of rtol 1e-5 (MSE tasks: d/dp of 2 (p - y) p (1 - p) is below 2.5 for y, p in [0, 1]: 2.5 times that)."""
    z, y, mse = _loss_inputs(T, B, mse_mask, Z_EDGES, lambda rng, s: rng.normal(0.0, 2.0, s))
    z64, y64 = z.astype(np.float64), y.astype(np.float64)
    p = (1.0 / (1.0 + np.exp(-z64))).astype(np.float32)
    z_d, p_d, y_d = (torch.from_numpy(a).to(dev) for a in (z, p, y))
    loss = torch.full((2,), SENT, device=dev)
    K.task_loss_logits_fwd(z_d, p_d, y_d, T, B, loss, device=dev, mse_mask=mse_mask)
    p64 = p.astype(np.float64)
    ref = sum(float(np.mean((p64[t] - y64[t]) ** 2)) if mse[t] else km.keras_bce_logits(y64[t], z64[t])
              for t in range(T))
    got = loss.cpu().numpy()
    assert got[1] == SENT and np.isfinite(got[0])
    np.testing.assert_allclose(got[0], ref, rtol=1e-5)

    gscale = 1.7
    zt = torch.from_numpy(z64).requires_grad_(True)
    yt = torch.from_numpy(y64)
    bce = torch.clamp(zt, min=0.0) - zt * yt + torch.log1p(torch.exp(-zt.abs()))
    per = torch.where(torch.from_numpy(mse)[:, None], (torch.sigmoid(zt) - yt) ** 2, bce)
    (per.mean(1).sum() * gscale).backward()
    dlogits = torch.full((T * B + 1,), SENT, device=dev)
    K.task_loss_logits_bwd(p_d, y_d, torch.tensor([gscale], device=dev), T, B, dlogits, mse_mask=mse_mask)
    got = dlogits.cpu().numpy()
    assert got[-1] == SENT and np.isfinite(got).all()
    np.testing.assert_allclose(got[:-1].reshape(T, B), zt.grad.numpy(), rtol=1e-5, atol=2.5 * 2.0 ** -24 * gscale / B)


# ---- ot_rows_colsum -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nrows', [0, 1, 33, 8225])
@pytest.mark.parametrize('ncols', [1, 20, 64, 300])
def test_rows_colsum(dev, ncols, nrows):
    """Column sums of a listed (permuted subset of a taller matrix, ld > ncols) or leading (rows = None) set of rows
    vs float64, written or accumulated; 8225 rows = 258 partials of 32 rows: the two-level reduce.  Two calls on
    the same input give the same bits."""
    rng = np.random.default_rng(ncols * 10000 + nrows)
    tall, ld = nrows + 50, ncols + 5
    src = rng.standard_normal((tall, ld)).astype(np.float32)
    rows = rng.permutation(tall)[:nrows].astype(np.int32)
    base = rng.standard_normal(ncols + 1).astype(np.float32)
    src_d = torch.from_numpy(src).to(dev)
    rows_d = torch.from_numpy(rows).to(dev) if nrows else torch.zeros(1, dtype=torch.int32, device=dev)
    for listed in (True, False):
        sel = src[rows] if listed else src[:nrows]
        ref = sel[:, :ncols].astype(np.float64).sum(0)
        for accumulate in (False, True):
            outs = []
            for _ in range(2):
                out = torch.from_numpy(base).to(dev)
                K.rows_colsum(src_d, ld, rows_d if listed else None, nrows, ncols, out, accumulate=accumulate,
                              device=dev)
                outs.append(out.cpu().numpy())
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
            assert outs[0][ncols] == base[ncols]
            np.testing.assert_allclose(outs[0][:ncols], ref + (base[:ncols].astype(np.float64) if accumulate else 0.0),
                                       rtol=1e-5, atol=1e-4)


# ---- tokenizer glue -------------------------------------------------------------------------------------------

NS_FIELD = np.dtype([('dense', '<u8'), ('ids', '<u8'), ('row_offset', '<i8'), ('stride', '<i8'), ('col', '<i4'),
                     ('width', '<i4')])


@pytest.mark.parametrize('B', [1, 257])
def test_ns_assemble_grad_pack(dev, B):
    """ot_ns_assemble / ot_ns_grad_pack vs numpy indexing, exactly: three id fields (row offsets 0, 11, 40 into one
    concatenated table) and two dense fields, interleaved in the output columns, read at element strides 4 and 3; the
    descriptors are laid out as OneTransModel._plan does (id fields first).  Columns past the fields keep their
    sentinel."""
    assert NS_FIELD.itemsize == NS_FIELD_BYTES
    rng = np.random.default_rng(B)
    W, vocab, offs = 6, [11, 29, 25], [0, 11, 40]
    table = rng.standard_normal((sum(vocab), W)).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab] + [np.full(B, -9)], 1).astype(np.int64)     # stride 4
    dense = rng.standard_normal((B, 3)).astype(np.float32)                                            # stride 3
    cols_s, cols_d = [0, W + 1, 2 * W + 2], [W, 2 * W + 1]
    F, ld = 3 * W + 2, 3 * W + 5
    ids_d, dense_d, table_d = (torch.from_numpy(a).to(dev) for a in (ids, dense, table))
    recs = np.zeros(5, NS_FIELD)
    for j in range(3):
        recs[j] = (0, ids_d.data_ptr() + 8 * j, offs[j], ids.shape[1], cols_s[j], W)
    for j in range(2):
        recs[3 + j] = (dense_d.data_ptr() + 4 * j, 0, 0, dense.shape[1], cols_d[j], 1)
    desc = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)

    out = torch.full((B, ld), SENT, device=dev)
    K.ns_assemble(desc, 5, table_d, B, out, ld)
    exp = np.full((B, ld), SENT, np.float32)
    for j in range(3):
        exp[:, cols_s[j]:cols_s[j] + W] = table[offs[j] + ids[:, j]]
    for j in range(2):
        exp[:, cols_d[j]] = dense[:, j]
    assert not (exp[:, :F] == SENT).any()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32))

    dmat = rng.standard_normal((B, ld)).astype(np.float32)
    keys = torch.full((3 * B + 1,), -5, dtype=torch.int64, device=dev)
    grads = torch.full((3 * B + 1, W), SENT, device=dev)
    K.ns_grad_pack(desc, 3, W, torch.from_numpy(dmat).to(dev), ld, B, keys, grads)
    exp_k = np.concatenate([offs[j] + ids[:, j] for j in range(3)] + [[-5]])
    exp_g = np.concatenate([dmat[:, cols_s[j]:cols_s[j] + W] for j in range(3)] + [np.full((1, W), SENT, np.float32)])
    assert np.array_equal(keys.cpu().numpy(), exp_k)
    assert np.array_equal(grads.cpu().numpy().view(np.uint32), exp_g.view(np.uint32))


@pytest.mark.parametrize('B', [1, 257])
def test_fill_rows_seq_rows(dev, B):
    """ot_fill_rows writes vec into the listed rows' first d columns and nothing else; ot_seq_rows copies the ids in
    [0, vocab) and maps the others (-1, vocab) to -1, reading samples stride_b > L apart."""
    rng = np.random.default_rng(50 + B)
    R, ld, d = 3 * B + 2, 24, 20
    rows = rng.permutation(R)[:B].astype(np.int32)
    vec = rng.standard_normal(d).astype(np.float32)
    dst = torch.full((R, ld), SENT, device=dev)
    K.fill_rows(dst, ld, torch.from_numpy(rows).to(dev), B, torch.from_numpy(vec).to(dev), d)
    exp = np.full((R, ld), SENT, np.float32)
    exp[rows, :d] = vec
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    K.fill_rows(dst, ld, torch.from_numpy(rows).to(dev), 0, torch.from_numpy(vec + 1).to(dev), d)    # no rows
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), exp.view(np.uint32))

    L, stride_b, vocab = 7, 10, 50
    ids = rng.integers(-1, vocab + 1, (B, stride_b)).astype(np.int64)
    ids[0, :3] = [-1, vocab, vocab - 1]
    ids[:, L:] = 3                                  # the gap between samples: valid ids that must not be read
    in_rows = torch.full((B * L + 1,), -9, dtype=torch.int32, device=dev)
    K.seq_rows(torch.from_numpy(ids).to(dev), stride_b, B, L, vocab, in_rows)
    got = in_rows.cpu().numpy()
    seen = ids[:, :L]
    assert got[-1] == -9 and got[:3].tolist() == [-1, -1, vocab - 1]
    assert np.array_equal(got[:-1].reshape(B, L), np.where((seen >= 0) & (seen < vocab), seen, -1))
