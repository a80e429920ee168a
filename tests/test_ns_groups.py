"""CPU: the group-wise NS tokenizer (``OneTransConfig.ns_tokenizer = 'group'``, paper eq. 6) — configuration, parameter
layout and clip units, the float64 yardstick tests/ns_groups_ref.py tied to the untouched oracle, and the argument
checks of the ot_ns_group_* entry points (which return before any launch, so they run without a GPU)."""

import copy
import json

import numpy as np
import pytest
import torch

import bag_ref as BR
import ns_groups_ref as NG
from recommend_amd import _lib
from recommend_amd.config import (OneTransConfig, check_ns_tokenizer, even_ns_groups, ns_group_layout,
                                  workload_config)
from recommend_amd.data import make_batch
from recommend_amd.layout import FlatLayout
from recommend_amd.params import dense_param_shapes, init_params, keras_variables
from oracle import onetrans_ref as R


def small(Lns=4, d=8, bags=False):
    cfg = workload_config('C2')
    cfg.hidden_dim, cfg.num_heads, cfg.ffn_dim, cfg.num_layers, cfg.num_ns_tokens = d, 2, 2 * d, 1, Lns
    cfg.sparse_features = {k: 40 + 7 * i for i, k in enumerate(cfg.sparse_features)}
    cfg.seq_item_vocab = 300
    cfg._seq_lens = [3, 2, 4]
    if bags:
        fc = cfg.feature_config
        fc['user_features'] = fc['user_features'][:2] + ['tags'] + fc['user_features'][2:]
        fc['context_features'] = fc['context_features'][:1] + ['sim_items'] + fc['context_features'][1:]
        cfg.bag_features = {'tags': {'cardinality': 23, 'pooling': 'sum'},
                            'sim_items': {'table': 'seq_item', 'pooling': 'mean'}}
    return NG.with_groups(cfg)


# =============================================================================== config
def test_default_is_auto_and_fields_round_trip():
    assert OneTransConfig().ns_tokenizer == 'auto' and OneTransConfig().ns_token_groups == []
    check_ns_tokenizer(OneTransConfig())
    cfg = small()
    back = OneTransConfig.from_dict(json.loads(json.dumps(cfg.to_dict())))
    assert back.ns_tokenizer == 'group' and back.ns_token_groups == cfg.ns_token_groups
    back.ns_token_groups[0].append('x')
    assert 'x' not in cfg.ns_token_groups[0]                               # a deep copy
    old = {k: v for k, v in cfg.to_dict().items() if k not in ('ns_tokenizer', 'ns_token_groups')}
    legacy = OneTransConfig.from_dict(old)
    assert legacy.ns_tokenizer == 'auto' and legacy.ns_token_groups == []
    check_ns_tokenizer(legacy)


@pytest.mark.parametrize('edit,match', [
    (lambda c: setattr(c, 'ns_tokenizer', 'mlp'), 'unknown ns_tokenizer'),
    (lambda c: setattr(c, 'ns_token_groups', []), 'needs ns_token_groups'),
    (lambda c: setattr(c, 'ns_token_groups', None), 'needs ns_token_groups'),
    (lambda c: c.ns_token_groups.pop(), 'num_ns_tokens is 4'),
    (lambda c: c.ns_token_groups.append(['I1']), 'num_ns_tokens is 4'),
    (lambda c: (c.ns_token_groups[1].extend(c.ns_token_groups[0]), c.ns_token_groups.__setitem__(0, [])), 'is empty'),
    (lambda c: c.ns_token_groups[1].append('ghost'), 'none of the user / item / context'),
    (lambda c: c.ns_token_groups[1].append(c.ns_token_groups[2][0]), 'is in groups 1 and 2'),
    (lambda c: c.ns_token_groups[1].append(c.ns_token_groups[1][0]), 'is in groups 1 and 1'),
    (lambda c: c.ns_token_groups[2].pop(), 'are in no group'),
])
def test_check_ns_tokenizer_refusals(edit, match):
    cfg = small()
    check_ns_tokenizer(cfg)
    edit(cfg)
    with pytest.raises(ValueError, match=match):
        check_ns_tokenizer(cfg)


@pytest.mark.parametrize('workload,L', [('C2', 12), ('C2', 5), ('C1', 8), ('C1', 11), ('C2', 39), ('C2', 1)])
def test_even_ns_groups_is_a_contiguous_near_even_partition(workload, L):
    cfg = workload_config(workload)
    cfg.num_ns_tokens = L
    groups = even_ns_groups(cfg)
    assert len(groups) == L and all(groups)
    assert [n for g in groups for n in g] == cfg.ns_feature_names()        # contiguous runs, in concat order
    cfg.ns_tokenizer, cfg.ns_token_groups = 'group', groups
    lay = ns_group_layout(cfg)
    assert lay['goff'][-1] == cfg.ns_input_width() and lay['widths'] == [cfg.ns_input_width(g) for g in groups]
    widest = max(cfg.ns_feature_width(n) for n in cfg.ns_feature_names())
    ideal = cfg.ns_input_width() / L
    if len(cfg.ns_feature_names()) >= 2 * L:      # near-equal: no cut is further than one feature from the ideal cut
        assert all(abs(lay['goff'][g] - g * ideal) <= widest for g in range(L + 1))
    cfg.num_ns_tokens = len(cfg.ns_feature_names()) + 1
    with pytest.raises(ValueError, match='cannot fill'):
        even_ns_groups(cfg)


# =============================================================================== parameters
def test_group_layout_rows_follow_concat_order_inside_each_group():
    cfg = small()
    lay = ns_group_layout(cfg)
    order = {n: i for i, n in enumerate(cfg.ns_feature_names())}
    assert lay['widths'][0] == 1                                           # the K_g = 1 group
    row = 0
    for g, members in enumerate(lay['members']):
        assert sorted(members, key=order.__getitem__) == members and set(members) == set(cfg.ns_token_groups[g])
        assert lay['goff'][g] == row
        for n in members:
            assert lay['col'][n] == row
            row += cfg.ns_feature_width(n)
    assert row == lay['goff'][-1] == cfg.ns_input_width()
    concat = [order[n] for members in lay['members'] for n in members]
    assert concat != sorted(concat)                                        # the groups are not contiguous runs


def test_init_params_shapes_draws_and_perturb():
    cfg = small()
    F, d, L = cfg.ns_input_width(), cfg.hidden_dim, cfg.num_ns_tokens
    P = init_params(cfg, F, seed=3, with_tables=False)
    assert P['tok.ns.kernel'].shape == (F, d) and P['tok.ns.bias'].shape == (L, d)
    assert not P['tok.ns.bias'].any()
    assert dense_param_shapes(cfg, F)['tok.ns.kernel'] == (F, d) and dense_param_shapes(cfg, F)['tok.ns.bias'] == (L, d)
    # one glorot(F_g, d) draw per group, in group order, in place of the single dense draw
    rng = np.random.Generator(np.random.PCG64(3))
    lay = ns_group_layout(cfg)
    for g, w in enumerate(lay['widths']):
        lim = np.sqrt(6.0 / (w + d))
        want = rng.uniform(-lim, lim, size=(w, d))
        assert np.array_equal(P['tok.ns.kernel'][lay['goff'][g]:lay['goff'][g + 1]], want)
    assert init_params(cfg, F, seed=3, perturb=True, with_tables=False)['tok.ns.bias'].all()
    auto = copy.copy(cfg)
    auto.ns_tokenizer = 'auto'
    Pa = init_params(auto, F, seed=3, with_tables=False)
    assert Pa['tok.ns.kernel'].shape == (F, L * d) and Pa['tok.ns.bias'].shape == (L * d,)
    with pytest.raises(ValueError, match='hold'):
        init_params(cfg, F - 1, seed=3, with_tables=False)


def test_keras_variables_one_kernel_and_one_bias_unit_per_group():
    cfg = small()
    F, d, L = cfg.ns_input_width(), cfg.hidden_dim, cfg.num_ns_tokens
    shapes = dense_param_shapes(cfg, F)
    kv = keras_variables(cfg, shapes)
    kern = [v for v in kv if v[0] == 'tok.ns.kernel']
    bias = [v for v in kv if v[0] == 'tok.ns.bias']
    assert len(kern) == L and len(bias) == L
    lay = ns_group_layout(cfg)
    covered = np.zeros(F * d, int)
    for g, (_, off, rows, cols, stride) in enumerate(kern):
        assert (off, rows, cols, stride) == (lay['goff'][g] * d, lay['widths'][g], d, d)
        covered[off:off + rows * cols] += 1
    assert np.all(covered == 1)                                            # the units tile the bank exactly
    covered = np.zeros(L * d, int)
    for (_, off, rows, cols, stride) in bias:
        assert (rows, cols) == (1, d)
        covered[off:off + cols] += 1
    assert np.all(covered == 1)
    auto = copy.copy(cfg)
    auto.ns_tokenizer = 'auto'
    kva = keras_variables(auto, dense_param_shapes(auto, F))
    assert len([v for v in kva if v[0].startswith('tok.ns.')]) == 2
    assert [v for v in kv if not v[0].startswith('tok.ns.')] == [v for v in kva if not v[0].startswith('tok.ns.')]


def test_flat_layout_keeps_the_bank_without_shadow_or_images():
    cfg = small(d=128)
    F = cfg.ns_input_width()
    lay = FlatLayout(cfg, F)
    assert lay.f_pad == (F + 3) // 4 * 4 and lay.shapes['tok.ns.kernel'] == (lay.f_pad, 128)
    assert lay.shapes['tok.ns.bias'] == (cfg.num_ns_tokens, 128)
    assert 'tok.ns.kernel' not in lay.gemm_banks
    assert not any(name == 'tok.ns.kernel' for (name, _) in lay.images)
    # the clip units of the flat buffer: the groups' kernels and biases, the padding rows in none of them
    o = lay.offsets['tok.ns.kernel']
    segs = [tuple(s) for s in lay.segments if o <= s[0] < o + lay.f_pad * 128]
    gl = ns_group_layout(cfg)
    assert segs == [(o + gl['goff'][g] * 128, gl['widths'][g], 128, 128) for g in range(cfg.num_ns_tokens)]
    auto = copy.copy(cfg)
    auto.ns_tokenizer = 'auto'
    la = FlatLayout(auto, F)
    assert 'tok.ns.kernel' in la.gemm_banks and ('tok.ns.kernel', 'fwd') in la.images
    with pytest.raises(ValueError, match='hold'):
        FlatLayout(cfg, F + 1)


# =============================================================================== the yardstick
def test_tokenizer_groups_equals_the_oracle_on_the_expanded_parameters():
    """Groups non-contiguous in concat order, one single-dense-feature group (K_g = 1) and groups that include bags:
    the grouped tokenizer equals the untouched oracle's tokenizer (through bag_ref, which feeds it the pooled bags)
    on the block-structured auto-split parameters, in float64."""
    cfg = small(bags=True)
    lay = ns_group_layout(cfg)
    assert lay['widths'][0] == 1
    bag_groups = {g for g, m in enumerate(lay['members']) for n in m if n in cfg.bag_features}
    assert bag_groups and all(len(lay['members'][g]) > 1 for g in bag_groups)
    P = init_params(cfg, cfg.ns_input_width(), seed=5, perturb=True)
    ns, seq, _ = make_batch(9, cfg, seed=77)
    assert set(cfg.bag_features) <= set(ns)
    Pt, nst, seqt = R.to_torch(P), R.to_torch(ns), R.to_torch(seq)
    got = NG.tokenizer_groups(Pt, cfg, nst, seqt)
    cfg_a, Pa = NG.expand_to_auto(cfg, P)
    assert Pa['tok.ns.kernel'].shape == (cfg.ns_input_width(), cfg.num_ns_tokens * cfg.hidden_dim)
    # block structure: a feature's rows are non-zero only in its group's column block
    nz = (Pa['tok.ns.kernel'].reshape(-1, cfg.num_ns_tokens, cfg.hidden_dim) != 0).any(axis=2).sum(axis=1)
    assert np.all(nz == 1)
    want = BR.tokenizer_bags(R.to_torch(Pa), cfg_a, nst, seqt)
    assert got.shape == want.shape == (9, sum(cfg._seq_lens) + 2 + cfg.num_ns_tokens, cfg.hidden_dim)
    assert (got - want).abs().max().item() < 1e-12
    assert got[:, -cfg.num_ns_tokens:].abs().max().item() > 1e-2
    # absent features leave their columns zero; a group with nothing present yields its bias
    gone = set(lay['members'][1])
    ns1 = {k: v for k, v in nst.items() if k not in gone and k[:-len('_weight')] not in gone}
    tok = NG.tokenizer_groups(Pt, cfg, ns1, seqt)
    assert torch.equal(tok[:, -cfg.num_ns_tokens + 1], Pt['tok.ns.bias'][1].expand(9, -1))
    assert torch.equal(tok[:, -cfg.num_ns_tokens], got[:, -cfg.num_ns_tokens])
    # no NS feature at all: the oracle's zero-token branch
    assert not NG.tokenizer_groups(Pt, cfg, {}, seqt)[:, -cfg.num_ns_tokens:].any()


# =============================================================================== ABI
def test_symbols_exist():
    lib = _lib.load()
    for name in ('ot_ns_group_fwd', 'ot_ns_group_bwd_input', 'ot_ns_group_bwd_weight',
                 'ot_ns_group_wgrad_workspace_size'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols()
    assert lib.ot_version() == 20000


def test_bad_arguments_return_the_error_status_before_any_launch():
    """Nothing here is a device pointer: a launch would fault."""
    f = 0x1000
    ws_need = _lib.size('ot_ns_group_wgrad_workspace_size', 37, 3, 10, 64)
    assert ws_need == 1 * (10 + 3) * 64 * 4                                # one row chunk: the dW and db slabs
    assert _lib.size('ot_ns_group_wgrad_workspace_size', 130, 3, 10, 64) == 2 * (10 + 3) * 64 * 4

    def fwd(A=f, goff=f, G=3, ktot=10, kmax=5, W=f, bias=f, B=37, d=64, X=f, lda=12, ldx=3 * 64):
        _lib.call('ot_ns_group_fwd', A, lda, goff, G, ktot, kmax, W, bias, B, d, X, ldx, None)

    def bwi(D=f, goff=f, G=3, ktot=10, kmax=5, W=f, B=37, d=64, dA=f, lda=12, ldd=3 * 64):
        _lib.call('ot_ns_group_bwd_input', D, ldd, goff, G, ktot, kmax, W, B, d, dA, lda, None)

    def bww(A=f, D=f, goff=f, G=3, ktot=10, kmax=5, B=37, d=64, dW=f, db=f, ws=f, nws=ws_need, lda=12, ldd=3 * 64):
        _lib.call('ot_ns_group_bwd_weight', A, lda, D, ldd, goff, G, ktot, kmax, B, d, dW, db, 0, ws, nws, None)

    for call, names in ((fwd, ('A', 'goff', 'W', 'bias', 'X')), (bwi, ('D', 'goff', 'W', 'dA')),
                        (bww, ('A', 'D', 'goff', 'dW', 'db'))):
        for n in names:
            with pytest.raises(_lib.OneTransHipError, match='null operand'):
                call(**{n: None})
        with pytest.raises(_lib.OneTransHipError, match=r'G=0 must be'):
            call(G=0)
        for d in (0, 6, 62, 516):
            with pytest.raises(_lib.OneTransHipError, match='multiple of 4'):
                call(d=d)
        with pytest.raises(_lib.OneTransHipError, match='B=0'):
            call(B=0)
        with pytest.raises(_lib.OneTransHipError, match='kmax'):
            call(kmax=0)
        with pytest.raises(_lib.OneTransHipError, match='kmax'):
            call(kmax=11)
        with pytest.raises(_lib.OneTransHipError, match='every group has a column'):
            call(ktot=2)
        with pytest.raises(_lib.OneTransHipError, match='lda'):
            call(lda=9)
    with pytest.raises(_lib.OneTransHipError, match='ldx'):
        fwd(ldx=3 * 64 - 4)
    with pytest.raises(_lib.OneTransHipError, match='ldx'):
        fwd(ldx=3 * 64 + 2)
    with pytest.raises(_lib.OneTransHipError, match='ldd'):
        bwi(ldd=100)
    with pytest.raises(_lib.OneTransHipError, match='16-byte aligned'):
        fwd(X=f + 4)
    with pytest.raises(_lib.OneTransHipError, match='workspace'):
        bww(nws=ws_need - 4)
    with pytest.raises(_lib.OneTransHipError, match='workspace'):
        bww(ws=None)
