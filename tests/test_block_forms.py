"""CPU: the block's form functions (block.block_fwd_form / block_bwd_form / ffn_bwd_rule) over a grid of modes, widths
and switches: the invariants the launches rely on.  No kernel runs: the model is a bare object with a layout whose
images count as built, and the capability queries are host-only functions of the library."""

import itertools

import pytest
import torch

from recommend_amd import kernels as K
from recommend_amd.block import FwdForm, block_bwd_form, block_fwd_form, ffn_bwd_rule
from recommend_amd.config import workload_config
from recommend_amd.layout import TILE, FlatLayout
from recommend_amd.model import OneTransModel

HEADS = {64: 4, 128: 4, 256: 4, 384: 6}
_LAYOUTS = {}


def bare_model(d, pair_dgrad, mode, fuse_bwd):
    """What the form functions read of a model, and nothing else: config, layout, the fuse switches."""
    if (d, pair_dgrad) not in _LAYOUTS:
        cfg = workload_config('C2')
        cfg.hidden_dim, cfg.num_heads, cfg.ffn_dim, cfg.num_layers, cfg.num_ns_tokens = d, HEADS[d], 2 * d, 2, 12
        cfg._seq_lens = [20, 20, 20]
        _LAYOUTS[(d, pair_dgrad)] = (cfg, FlatLayout(cfg, cfg.ns_input_width(), pair_dgrad=pair_dgrad))
    m = OneTransModel.__new__(OneTransModel)
    torch.nn.Module.__init__(m)
    m.config, m.layout = _LAYOUTS[(d, pair_dgrad)]
    m.img, m._img_valid, m._img_mode = torch.zeros(1, dtype=torch.int16), True, mode     # images "built": no launch
    m.attn_fp8, m._aux_maps = False, {}
    m.fuse_norms = m.fuse_bwd2 = d % TILE == 0
    m.fuse_bwd = fuse_bwd and d == TILE
    return m


GRID = list(itertools.product(('split', 'f32', 'bf16'), (64, 128, 256, 384), (0.0, 0.1), (False, True), (False, True),
                              (False, True), (False, True)))


@pytest.mark.parametrize('mode,d', [(mode, d) for mode in ('split', 'f32', 'bf16') for d in (64, 128, 256, 384)])
def test_form_invariants(mode, d):
    I = 12 + 3 * 20 + 2
    seen = set()
    for _, _, rate, masked, pair_dgrad, fuse_bwd, has_bounds in [g for g in GRID if g[:2] == (mode, d)]:
        m = bare_model(d, pair_dgrad, mode, fuse_bwd)
        f = m.config.ffn_dim
        with K.precision(mode):
            for l, Kq, need_out in ((0, I, True), (1, 1, True), (1, 1, False)):
                fwd = block_fwd_form(m, l, I, Kq, rate > 0, False, masked, need_out=need_out)
                assert isinstance(fwd, FwdForm)
                with pytest.raises(AttributeError):
                    fwd.h = True                                            # immutable
                # a fused FFN forward => pair-form W2 => no stored bf16 h; u_bf => h
                assert not fwd.ffn_fused or fwd.pair_w2
                assert not fwd.pair_w2 or not fwd.h
                assert not fwd.u_bf or fwd.h
                assert not fwd.ffn_fused or (need_out and d == TILE)
                assert fwd.write_u and (fwd.fold is None or (Kq == 1 and not masked))
                u_bound = has_bounds and fwd.pair_w2                        # (the forward takes |U| exactly there)
                bwd = block_bwd_form(m, l, I, Kq, rate, masked, has_bounds, u_bound, fwd)
                # mask_fused => ffn_bwd => both FFN dgrad images in the pair form, d == 128, f % 128 == 0
                assert not bwd.mask_fused or bwd.ffn_bwd
                assert not bwd.ffn_bwd or (bwd.pw2 and bwd.pw1 and d == TILE and f % TILE == 0)
                assert not bwd.mask_fused or (rate > 0 and has_bounds and not masked)
                assert not bwd.du_bf or not bwd.ffn_bwd
                assert not bwd.ffn_bwd or bwd.dx1_ep
                # no row maxima asked of a dropout pass that cannot report them
                assert not bwd.dy2_rowmax or K.dropout_rowmax_supported(d)
                assert not (bwd.dy2_rowmax or bwd.dy2_bound) or (rate > 0 and not bwd.mask_fused)
                assert not bwd.rep_dx or (bwd.pqkv and bwd.qkv_ep)
                if l == 1:
                    # block 1's question about block 0 = block 0's own rule, and its own form, with no padding mask
                    fwd0 = block_fwd_form(m, 0, I, I, rate > 0, False, False)
                    own = block_bwd_form(m, 0, I, I, rate, False, has_bounds, has_bounds and fwd0.pair_w2, fwd0)
                    assert bwd.rep_dx == (bwd.pqkv and ffn_bwd_rule(m, 0, rate, has_bounds, False)[1])
                    assert bwd.rep_dx == (bwd.pqkv and own.mask_fused)
                seen.add((fwd.ffn_fused, bwd.ffn_bwd, bwd.mask_fused))
    if mode == 'split' and d == TILE:       # the grid reaches the fused forms, with and without the mask, and neither
        assert {(True, True, True), (True, True, False), (True, False, False)} <= seen
    else:
        assert seen == {(False, False, False)}


def test_forms_follow_live_switches():
    """Forms are evaluated at call time: a switch flipped on a live model changes the next form."""
    m = bare_model(128, True, 'split', True)
    I = 74
    with K.precision('split'):
        assert ffn_bwd_rule(m, 0, 0.1, True, False) == (True, True)
        assert ffn_bwd_rule(m, 0, 0.1, True, True) == (True, False)          # a padding mask: the dropout pass
        assert ffn_bwd_rule(m, -1, 0.1, True, False) == (False, False)       # block 0 has no block below
        old = K.bwd_mask_fused(0)
        try:
            assert ffn_bwd_rule(m, 0, 0.1, True, False) == (True, False)
        finally:
            K.bwd_mask_fused(old)
        old = K.ffn_fused(0)
        try:
            assert not block_fwd_form(m, 0, I, I, True, False, False).ffn_fused
        finally:
            K.ffn_fused(old)
        assert block_fwd_form(m, 0, I, I, True, False, False).ffn_fused
        m.fuse_bwd = False
        assert ffn_bwd_rule(m, 0, 0.1, True, False) == (False, False)
