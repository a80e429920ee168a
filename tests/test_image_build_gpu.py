"""ot_split_images: the one-launch build (ot_image_build 1, build_images_kernel) against the two-launch reference
path (ot_image_build 0: image_colscale_kernel + split_images_kernel).  The requirement is byte identity of the whole
image buffer: both buffers start from the same 0xA5 pattern (with one spare unit behind the image), so the planes a
pair image leaves unwritten, the tag and any stray write show up.

Shapes: both orientations (n contiguous: sn = 1, sk = N; k contiguous: sn = K, sk = 1), the three forms (kscale -1:
split8, -2: pair, a gamma offset: gamma-folded pair), both precisions, G in {1, 3}, N in {128, 256, 200} (200: a partial
second column tile), K in {16, 48, 512}; a source offset that is no multiple of four floats takes the scalar loads.
The scale cases check pow2_scale14's contract on the column maxima directly (an independent integer model of it)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from recommend_amd import kernels as K
from recommend_amd.layout import IMAGE_UNIT_ELEMS

PATTERN = -23131          # 0xA5A5 as int16


@pytest.fixture
def switch(dev):
    prev = K.image_build(-1)
    yield
    K.image_build(prev)


@pytest.fixture(params=['split', 'bf16'])
def precision(dev, request):
    old = K.set_matmul_mode(request.param)
    yield request.param
    K.set_matmul_mode(old)


def units_of(G, N, K_):
    return G * ((N + 127) // 128) * (K_ // 16)


def bank(orient, G, N, K_, src_off, kscale, dst_off, first_unit):
    """One descriptor row for B[g][n][k] stored n-contiguous ('n': [g][k][n]) or k-contiguous ('k': [g][n][k])."""
    sn, sk = (1, N) if orient == 'n' else (K_, 1)
    return [src_off, sn, sk, N * K_, kscale, dst_off, first_unit, G, N, K_]


def build(dev, base, desc, total_units, image_units, mode):
    """The image buffer (plus one spare unit) after one ot_split_images call with the switch at ``mode``."""
    K.image_build(mode)
    img = torch.full(((image_units + 1) * IMAGE_UNIT_ELEMS,), PATTERN, dtype=torch.int16, device=dev)
    d = torch.tensor(desc, dtype=torch.int64, device=dev).reshape(-1)
    K.split_images(base, d, len(desc), total_units, img)
    torch.cuda.synchronize()
    return img


def both(dev, base, desc, total_units, image_units=None):
    image_units = total_units if image_units is None else image_units
    ref = build(dev, base, desc, total_units, image_units, 0)
    new = build(dev, base, desc, total_units, image_units, 1)
    assert torch.equal(ref[image_units * IMAGE_UNIT_ELEMS:], torch.full_like(ref[:IMAGE_UNIT_ELEMS], PATTERN))
    assert torch.equal(new, ref), f'{int((new != ref).sum())} of {new.numel()} image elements differ'
    return new


_BASE = {}


def weights(dev, n, seed=0):
    """Seeded random weights whose columns span several binades, built once per size and never written."""
    if (n, seed) not in _BASE:
        gen = torch.Generator().manual_seed(seed)
        w = torch.randn(n, generator=gen) * 10.0 ** (-3 * torch.rand(n, generator=gen))
        _BASE[(n, seed)] = w.float().to(dev)
    return _BASE[(n, seed)]


@pytest.mark.parametrize('K_', [16, 48, 512])
@pytest.mark.parametrize('N', [128, 256, 200])
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('form', ['split8', 'pair', 'gamma'])
@pytest.mark.parametrize('orient', ['n', 'k'])
def test_single_bank_bytes(dev, switch, precision, orient, form, G, N, K_):
    nw = G * N * K_
    base = weights(dev, 3 * 256 * 512 + 512 + 64)
    kscale = {'split8': -1, 'pair': -2, 'gamma': 3 * 256 * 512}[form]          # gamma: 16-B aligned, past every bank
    assert nw <= 3 * 256 * 512
    u = units_of(G, N, K_)
    assert K.split_image_elems(G, N, K_) == u * IMAGE_UNIT_ELEMS
    both(dev, base, [bank(orient, G, N, K_, 0, kscale, 0, 0)], u)


@pytest.mark.parametrize('orient', ['n', 'k'])
@pytest.mark.parametrize('src_off,gamma_off', [(3, 40000), (0, 40001), (8, 40002)])
def test_unaligned_offsets_bytes(dev, switch, precision, orient, src_off, gamma_off):
    """Offsets that break the 16-byte alignment of the bank or of gamma: the scalar loads, same bytes."""
    base = weights(dev, 3 * 256 * 512 + 512 + 64)
    G, N, K_ = 2, 200, 48
    both(dev, base, [bank(orient, G, N, K_, src_off, gamma_off, 0, 0)], units_of(G, N, K_))


def test_strided_bank_bytes(dev, switch, precision):
    """Neither axis contiguous (sn = 2 K, sk = 2): the general form of the descriptor."""
    base = weights(dev, 3 * 256 * 512 + 512 + 64)
    G, N, K_ = 2, 136, 32
    both(dev, base, [[4, 2 * K_, 2, 2 * N * K_, -2, 0, 0, G, N, K_]], units_of(G, N, K_))


def mixed_descs():
    shapes = [('n', 2, 256, 48, -1), ('k', 1, 200, 512, 'gamma'), ('n', 3, 128, 16, -2), ('k', 2, 384, 64, -2),
              ('n', 1, 128, 128, 'gamma'), ('k', 1, 128, 32, -1)]
    desc, src, units = [], 0, 0
    gamma_off = sum(G * N * K_ for _, G, N, K_, _ in shapes)
    for orient, G, N, K_, ks in shapes:
        desc.append(bank(orient, G, N, K_, src, gamma_off if ks == 'gamma' else ks, units * IMAGE_UNIT_ELEMS, units))
        src += G * N * K_
        units += units_of(G, N, K_)
    return desc, gamma_off + 512, units


def test_mixed_banks_bytes(dev, switch, precision):
    """Six banks of the three forms with different G / N / K in one call: the descriptor lookup at every bank boundary
    and the last unit."""
    desc, nbase, units = mixed_descs()
    both(dev, weights(dev, nbase, seed=1), desc, units)


@pytest.mark.parametrize('short', [1, 3, 40])
def test_total_units_cuts_the_last_banks(dev, switch, precision, short):
    """total_units below the banks' sum: the units past it stay unwritten (also the scales of a tile whose first unit
    is past it), as with one workgroup per unit."""
    desc, nbase, units = mixed_descs()
    both(dev, weights(dev, nbase, seed=1), desc, units - short, image_units=units)


def test_no_units_writes_nothing(dev, switch, precision):
    base = weights(dev, 4096)
    for mode in (0, 1):
        img = build(dev, base, [bank('n', 1, 128, 16, 0, -2, 0, 0)], 0, 1, mode)
        assert bool((img == PATTERN).all())


# ------------------------------------------------------------------------------------------------ the scales
def pow2_scale14_model(m):
    """The contract of pow2_scale14 on one float32 maximum, on its bits: 2^(13 - floor(log2 m)) clamped to the normal
    range, 1 for zero and denormals, NaN for inf."""
    e = (np.float32(m).view(np.uint32) >> 23) & 255
    if e == 255:
        return np.float32(np.nan)
    se = 127 if e == 0 else min(254, max(1, 127 + 13 - (int(e) - 127)))
    return np.uint32(se << 23).view(np.float32)


def scales_of(img, tile_first_unit=0):
    o = tile_first_unit * IMAGE_UNIT_ELEMS + 2 * 128 * 16
    raw = img[o:o + 258].cpu().numpy().view(np.uint32)
    assert raw[128] == 0x7FC17FC1
    return raw[:128].view(np.float32)


def below(x):
    return np.nextafter(np.float32(x), np.float32(0))


@pytest.mark.parametrize('orient', ['n', 'k'])
def test_scale_values(dev, switch, orient):
    """Column maxima at chosen values: zero, a denormal, exact powers of two and the floats just below them at the
    exponent boundaries and at both clamps of the scale's exponent."""
    old = K.set_matmul_mode('split')
    try:
        N, K_ = 128, 64
        maxima = [0.0, 1e-40, below(2.0 ** -126)]
        for k in (-126, -125, -115, -114, -113, -20, -1, 0, 1, 13, 14, 15, 100, 127):
            maxima += [np.float32(2.0 ** k), below(2.0 ** k) if k > -126 else np.float32(2.0 ** k)]
        maxima.append(np.finfo(np.float32).max)
        rng = np.random.default_rng(5)
        B = np.zeros((N, K_), np.float32)
        for n in range(N):
            m = np.float32(maxima[n % len(maxima)])
            B[n] = m * rng.uniform(0, 0.999, K_).astype(np.float32)          # below m in magnitude (m * [0, 1))
            B[n, rng.integers(K_)] = m if n % 2 else -m
        W = B if orient == 'k' else B.T
        base = torch.from_numpy(np.ascontiguousarray(W).reshape(-1)).to(dev)
        img = both(dev, base, [bank(orient, 1, N, K_, 0, -2, 0, 0)], units_of(1, N, K_))
        got = scales_of(img)
        want = np.array([pow2_scale14_model(np.abs(B[n]).max()) for n in range(N)], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got[0] == 1.0 and got[1] == 1.0
    finally:
        K.set_matmul_mode(old)


@pytest.mark.parametrize('orient', ['n', 'k'])
@pytest.mark.parametrize('bad', ['inf', '-inf', 'nan'])
def test_inf_and_nan_weights(dev, switch, orient, bad):
    """An infinite weight gives the NaN scale in its column only; a NaN weight is dropped from the maximum (fmaxf) and
    handed on by pair8: bytes equal to the reference path's either way."""
    old = K.set_matmul_mode('split')
    try:
        N, K_, col, k = 256, 48, 131, 17
        B = np.random.default_rng(9).standard_normal((N, K_)).astype(np.float32)
        B[col, k] = np.float32(bad)
        W = B if orient == 'k' else B.T
        base = torch.from_numpy(np.ascontiguousarray(W).reshape(-1)).to(dev)
        img = both(dev, base, [bank(orient, 1, N, K_, 0, -2, 0, 0)], units_of(1, N, K_))
        got = np.concatenate([scales_of(img, 0), scales_of(img, K_ // 16)])
        Bm = np.where(np.isnan(B), 0, np.abs(B))
        want = np.array([pow2_scale14_model(Bm[n].max()) for n in range(N)], np.float32)
        if bad == 'nan':
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        else:
            assert np.isnan(got[col]) and np.isnan(want[col])
            keep = np.arange(N) != col
            assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    finally:
        K.set_matmul_mode(old)


# ------------------------------------------------------------------------------------------------ model level
def train_three_steps(dev, mode):
    from recommend_amd.config import workload_config
    from recommend_amd.data import make_batch
    from recommend_amd.model import OneTransModel
    from recommend_amd.params import init_params
    from recommend_amd.trainer import OneTransTrainer
    K.image_build(mode)
    cfg = workload_config('C2')
    cfg.hidden_dim, cfg.num_heads, cfg.ffn_dim, cfg.num_layers, cfg.num_ns_tokens = 128, 4, 256, 2, 12
    cfg.sparse_features = {k: 40 + 7 * i for i, k in enumerate(cfg.sparse_features)}
    cfg.seq_item_vocab = 300
    cfg._seq_lens = [20, 20, 20]
    P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
    model = OneTransModel(cfg, device=str(dev), init=P)
    tr = OneTransTrainer(cfg, model=model)
    assert model.img is not None and model.layout.pair_images
    out = []
    for step in range(3):
        tr.train_step(make_batch(37, cfg, seed=1000 + step))
        torch.cuda.synchronize()
        out.append((model.img.clone(), {n: model.g(n).detach().clone() for n in model.layout.shapes}))
    return out


def test_model_images_and_gradients(dev, switch):
    """2 layers, d 128, B 37, split mode, three train steps under each switch value: the image buffer after every step
    is byte-equal and every gradient bank bit-equal."""
    old = K.set_matmul_mode('split')
    try:
        ref, new = train_three_steps(dev, 0), train_three_steps(dev, 1)
    finally:
        K.set_matmul_mode(old)
    for step, ((img0, g0), (img1, g1)) in enumerate(zip(ref, new)):
        assert torch.equal(img1, img0), f'step {step}: images differ'
        for n in g0:
            assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), f'step {step}: {n}'
