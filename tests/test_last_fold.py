"""The folded one-query attention's algebra in float64: the fold formulas of tests/fold_ref.py equal the
unfolded attention built from the same tensors (K / V projected for every row, softmax, PV, autograd), and the ``fold``
row map holds the rows the kernels and GEMMs address."""

import numpy as np
import pytest
import torch

from recommend_amd.config import workload_config
from recommend_amd.layout import layer_maps

import fold_ref as F

TOL = 1e-10


def dedicated_range(cfg, I):
    ded = [p for p in range(I) if cfg.group_of_position(p, I) != 0]
    assert ded == list(range(ded[0], ded[-1] + 1))
    return ded[0], ded[-1] + 1


def small_cfg(dedicated, Lns=4):
    cfg = workload_config('C2')
    cfg.num_ns_tokens, cfg.dedicated_positions = Lns, dedicated
    return cfg


@pytest.mark.parametrize('dedicated', ['head', 'tail'])
@pytest.mark.parametrize('H,hd', [(4, 8), (2, 16)])
def test_fold_equals_unfolded(dedicated, H, hd):
    I, B = 11, 3
    ded = dedicated_range(small_cfg(dedicated), I)
    c = F.make_case(B, I, H, hd, ded, seed=17 + H)
    S, D = c['S'], c['D']
    rstd = F.rstd_of(c['x'])
    xh = c['x'] * rstd[..., None]
    fwd = F.fold_forward(xh, c['gamma'], c['Wk0'], c['Wv0'], c['q'], c['Kd'], c['Vd'], S, D, H)
    bwd = F.fold_backward(xh, rstd, c['gamma'], c['Wk0'], c['Wv0'], c['q'], c['Kd'], c['Vd'], S, D, H, fwd, c['do'])
    ref = F.unfolded(c['x'], c['gamma'], c['Wk0'], c['Wv0'], c['q'], c['Kd'], c['Vd'], S, D, H, c['do'])
    assert (I - 1 in D) == (dedicated == 'tail')                  # the query is a shared key under 'head' only
    for name, got in (('o', fwd['o']), ('lse', fwd['lse']), ('dx', bwd['dx'][:, S]), ('dq', bwd['dq']),
                      ('dKd', bwd['dKd']), ('dVd', bwd['dVd']), ('dWk0', bwd['dWk0']), ('dWv0', bwd['dWv0']),
                      ('dgamma', bwd['dgamma'])):
        want = ref[name][:, S] if name == 'dx' else ref[name]
        err = (got - want).abs().max().item()
        assert err < TOL, f'{name}: {err:.2e}'
    assert bwd['dx'][:, D].abs().max().item() == 0


@pytest.mark.parametrize('dedicated', ['head', 'tail'])
def test_fold_map_rows(dedicated):
    """Space 0: the token rows of the dedicated positions and of the query, by weight group; space 1: the compact
    dqkv rows b*nf + (p - first dedicated), the query behind them when it is no dedicated key."""
    cfg = small_cfg(dedicated)
    B, I = 5, 13
    ded0, ded1 = dedicated_range(cfg, I)
    maps = layer_maps(cfg, B, I, 1)
    fm = maps['fold']
    q_ded = ded0 <= I - 1 < ded1
    nf = (ded1 - ded0) + (0 if q_ded else 1)
    assert fm.nrows == B * nf and len(fm.rows) == 2
    seen = set()
    for t in range(fm.ntiles):
        g = int(fm.tile_group[t])
        for tok, cmp_ in zip(fm.rows[0][t * 128:(t + 1) * 128], fm.rows[1][t * 128:(t + 1) * 128]):
            if tok < 0:
                assert cmp_ < 0
                continue
            b, p = divmod(int(tok), I)
            assert cfg.group_of_position(p, I) == g
            assert ded0 <= p < ded1 or p == I - 1
            assert cmp_ == b * nf + (p - ded0 if ded0 <= p < ded1 else ded1 - ded0)
            seen.add((b, p))
    assert len(seen) == B * nf
    assert 'fold' not in layer_maps(cfg, B, I, 4) and 'fold' not in layer_maps(cfg, B, I, I)
    # the other maps are what they were
    assert maps['all'].nrows == B * I and maps['tail'].nrows == B
