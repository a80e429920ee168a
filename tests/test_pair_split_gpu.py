"""The scaled fp16-pair split of the pair GEMMs (csrc/common.h pair8 / pair4) and of the slice attention (its residual
by pair_lo_mix) against its definition, bit for bit.

With t = float32(x * s):  h = float16(t) (pair8: t saturated to [-65504, 65504] first), l = float16(t - float32(h)),
both rounded to nearest even.  ``ot_pair_split_probe`` writes the two planes of a flat vector; numpy forms the same
planes on the CPU.  One vector of a few thousand values holds random normals at several magnitudes, exact fp16
rounding ties of t (towards and away from zero) and of the residual, residuals in the fp16 subnormal range and below
half its smallest subnormal, +-0, values past the fp16 range (the saturation), +-inf and NaN.  A NaN must stay a
NaN (compared with isnan); everything else is compared by bit pattern.  The CPU test checks that the constructed
ties and subnormals are what they claim to be.
"""

import functools

import numpy as np
import pytest

F16_MAX = 65504.0
SCALES = (32.0, 0.25)          # powers of two, as pow2_scale14 gives: t = x * s is exact


def _f16(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16)


@functools.lru_cache(maxsize=None)
def make_inputs(scale: float):
    """(x float32 [n], groups: name -> slice into x).  Built in t = x * scale space and divided by the scale."""
    rng = np.random.default_rng(20260116)
    parts, groups, n = [], {}, 0

    def add(name, t):
        nonlocal n
        t = np.asarray(t, dtype=np.float64)
        groups[name] = slice(n, n + t.size)
        parts.append(t)
        n += t.size

    add('normal', np.concatenate([rng.standard_normal(512) * m for m in (1e-3, 1.0, 100.0, 1e4)]).astype(np.float32))
    # t halfway between two neighbouring normal fp16 values a < b (bit patterns k, k + 1), both signs: k even rounds
    # towards zero (to a), k odd away from it (to b)
    k = rng.integers(0x2c00, 0x7bfe, size=256).astype(np.uint16)         # 2^-4 <= a < 65504
    k[:128] &= 0xfffe
    k[128:] |= 1
    a, b = _f16(k).astype(np.float64), _f16(k + 1).astype(np.float64)
    sign = np.where(np.arange(256) % 2 == 0, 1.0, -1.0)
    add('tie_h', sign * (a + b) / 2)
    # t = h + r with r halfway between two neighbouring normal fp16 values and below half an ulp of h: 11 bits of h and
    # 12 of r end 23 binary places below h's leading bit, so t is an exact float32
    e = rng.integers(-2, 15, size=256)
    h = np.ldexp(1.0 + rng.integers(1, 1024, size=256) / 1024.0, e)
    r = np.ldexp(1.0 + (2 * rng.integers(0, 1024, size=256) + 1) / 2048.0, e - 12)
    add('tie_l', sign * (h + np.where(np.arange(256) % 4 < 2, r, -r)))
    # residuals in the fp16 subnormal range [2^-24, 2^-14): h in [2^-3, 2^-2) (float32 spacing 2^-26), r = j 2^-26
    h = np.ldexp(1.0 + rng.integers(1, 1024, size=256) / 1024.0, -3)
    j = rng.integers(4, 1 << 12, size=256)
    j[:64] = 4 * rng.integers(1, 1 << 10, size=64) + 2                   # ties between two subnormals
    add('sub_l', sign * (h + np.where(np.arange(256) % 4 < 2, j, -j) * 2.0 ** -26))
    # residuals of 2^-26 (below half the smallest subnormal 2^-24: l = +-0) and of exactly half (2^-25: a tie, to 0)
    h = np.ldexp(1.0 + rng.integers(1, 1024, size=128) / 1024.0, -3)
    j = np.where(np.arange(128) < 64, 1.0, 2.0) * np.where(np.arange(128) % 4 < 2, 1.0, -1.0)
    add('tiny_l', sign[:128] * (h + j * 2.0 ** -26))
    add('zero', [0.0, -0.0] * 8)
    past = np.array([65505.0, 65510.0, 65519.0, 65520.0, 65536.0, 70000.0, 1e6, 1e30], dtype=np.float32)
    add('past', np.concatenate([past, -past]))
    add('inf', [np.inf, -np.inf] * 4)
    add('nan', [np.nan] * 8)
    t = np.concatenate(parts)
    assert t.size % 8 == 0 and 2000 < t.size < 8000
    x = (t / scale).astype(np.float32)
    with np.errstate(invalid='ignore'):
        ok = (x.astype(np.float64) * scale == t) | np.isnan(t)
    assert ok.all(), 'x * scale must reproduce t exactly'
    x.setflags(write=False)
    return x, groups


def reference(x, scale, saturate):
    """(h, l) as uint16 bit patterns, from the definition."""
    with np.errstate(over='ignore', invalid='ignore'):
        t = x.astype(np.float32) * np.float32(scale)
        if saturate:
            t = np.minimum(np.maximum(t, np.float32(-F16_MAX)), np.float32(F16_MAX))   # a NaN stays a NaN
        h = t.astype(np.float16)
        l = (t - h.astype(np.float32)).astype(np.float16)
    return h.view(np.uint16), l.view(np.uint16)


def _neighbours(v16):
    """The fp16 values just below and above v (float64), for finite v."""
    v = v16.astype(np.float16)
    return (np.nextafter(v, np.float16(-np.inf)).astype(np.float64), np.nextafter(v, np.float16(np.inf)).astype(np.float64))


@pytest.mark.parametrize('scale', SCALES)
def test_inputs_are_what_they_claim(scale):
    x, g = make_inputs(scale)
    t = x.astype(np.float64) * scale
    hb, lb = reference(x, scale, True)
    h, l = hb.view(np.float16).astype(np.float64), lb.view(np.float16).astype(np.float64)
    r = t - h                                                     # exact in float64 (and in float32)
    assert np.array_equal((t - h).astype(np.float32).astype(np.float64)[np.isfinite(t)], r[np.isfinite(t)])

    s = g['tie_h']                                                # t is the midpoint of h and h's other neighbour
    dn, up = _neighbours(hb[s].view(np.float16))
    other = np.where(np.abs(t[s]) > np.abs(h[s]), np.where(t[s] > 0, up, dn), np.where(t[s] > 0, dn, up))
    assert np.array_equal(t[s] - h[s], other - t[s]) and np.all(r[s] != 0)
    assert np.all(hb[s] & 1 == 0)                                 # to even ...
    toward = np.abs(h[s]) < np.abs(t[s])
    assert toward.sum() >= 64 and (~toward).sum() >= 64           # ... in both directions
    assert np.array_equal(l[s], r[s])                             # half an ulp of h is an exact fp16

    s = g['tie_l']                                                # r is the midpoint of l and l's other neighbour
    dn, up = _neighbours(lb[s].view(np.float16))
    other = np.where(l[s] < r[s], up, dn)
    assert np.all(l[s] != r[s]) and np.array_equal(r[s] - l[s], other - r[s])
    assert np.all(lb[s] & 1 == 0) and np.all(np.abs(l[s]) >= 2.0 ** -14)
    assert (np.abs(l[s]) < np.abs(r[s])).sum() >= 32 and (np.abs(l[s]) > np.abs(r[s])).sum() >= 32

    s = g['sub_l']
    assert np.all((np.abs(r[s]) >= 2.0 ** -24) & (np.abs(r[s]) < 2.0 ** -14))
    assert np.all(np.abs(l[s]) <= 2.0 ** -14) and np.all((lb[s] & 0x7c00 == 0) | (np.abs(l[s]) == 2.0 ** -14))
    ties = np.abs(np.abs(r[s]) - np.abs(l[s])) == 2.0 ** -25
    assert ties.sum() >= 64 and np.all(lb[s][ties] & 1 == 0)

    s = g['tiny_l']
    assert np.all((r[s] != 0) & (np.abs(r[s]) <= 2.0 ** -25))
    assert set(np.unique(np.abs(r[s]))) == {2.0 ** -26, 2.0 ** -25}
    assert np.all(lb[s] & 0x7fff == 0) and np.array_equal(lb[s] >> 15, (r[s] < 0).astype(np.uint16))

    s = g['zero']
    assert np.array_equal(hb[s], np.array([0, 0x8000] * 8, np.uint16)) and np.all(lb[s] == 0)
    s = g['past']
    assert np.all(np.abs(t[s]) > F16_MAX) and np.all(hb[s] & 0x7fff == 0x7bff) and np.all(lb[s] == 0)
    hu, lu = reference(x, scale, False)                           # without the saturation
    assert np.all(hu[s][3:8] == 0x7c00) and np.all(hu[s][:3] == 0x7bff) and np.all(lu[s][:3] != 0)
    s = g['inf']
    assert np.all(hb[s] & 0x7fff == 0x7bff) and np.all(lb[s] == 0)
    s = g['nan']
    assert np.all(np.isnan(hb[s].view(np.float16))) and np.all(np.isnan(lb[s].view(np.float16)))


@pytest.mark.gpu
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('form', ['pair8', 'pair4', 'slice'])
def test_pair_split_bits(dev, form, scale):
    import torch
    from recommend_amd import kernels as K
    x, groups = make_inputs(scale)
    hw, lw = reference(x, scale, saturate=(form == 'pair8'))
    hi, lo = K.pair_split_probe(torch.from_numpy(x.copy()).to(dev), scale, form)
    torch.cuda.synchronize()
    hg, lg = hi.cpu().numpy().view(np.uint16), lo.cpu().numpy().view(np.uint16)
    for name, want, got in (('h', hw, hg), ('l', lw, lg)):
        nan = np.isnan(want.view(np.float16))
        assert np.all(np.isnan(got.view(np.float16)[nan])), f'{form} {name}: a NaN did not stay a NaN'
        bad = np.flatnonzero((want != got) & ~nan)
        where = sorted({n for n, s in groups.items() for i in bad[:8] if s.start <= i < s.stop})
        assert bad.size == 0, (f'{form} {name}: {bad.size} differ, first at {bad[:8]} in {where}: x {x[bad[:8]]}, '
                               f'want {want[bad[:8]]}, got {got[bad[:8]]}')
