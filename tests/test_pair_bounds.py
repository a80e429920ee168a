"""CPU: the per-forward fp16-pair bounds object (model.PairBounds) and the read-only ``pair_dgrad`` switch."""

import pytest
import torch

from recommend_amd.config import workload_config
from recommend_amd.layout import FlatLayout
from recommend_amd.model import OneTransModel, PairBounds


def test_get_returns_only_what_a_producer_took():
    b = PairBounds(3, 'cpu')
    assert b.t.shape == (3, 8) and not b.t.any()
    assert all(b.get(l, n) is None for l in range(3) for n in PairBounds.SLOTS)
    v = b.out(1, 'u')
    assert v.shape == (1,) and b.get(1, 'u') is v and b.out(1, 'u') is v     # (the recompute takes it again)
    assert b.get(0, 'u') is None and b.get(1, 'o') is None
    v.fill_(3.0)
    assert b.t[1, PairBounds.SLOTS.index('u')].item() == 3.0 and b.t.sum().item() == 3.0


def test_slots_do_not_alias():
    b = PairBounds(2, 'cpu')
    views = [b.out(l, n) for l in range(2) for n in PairBounds.SLOTS]
    assert len({v.data_ptr() for v in views}) == len(views)
    for i, v in enumerate(views):
        v.fill_(i + 1.0)
    assert [v.item() for v in views] == [i + 1.0 for i in range(len(views))]
    with pytest.raises(ValueError):
        b.out(0, 'x')


def test_created_only_where_a_backward_can_use_it():
    assert isinstance(PairBounds.begin(2, 'cpu', 'split', True), PairBounds)
    assert PairBounds.begin(2, 'cpu', 'split', False) is None              # ONETRANS_PAIR_WGRAD=0
    assert PairBounds.begin(2, 'cpu', 'bf16', True) is None
    assert PairBounds.begin(2, 'cpu', 'f32', True) is None
    with torch.no_grad():
        assert PairBounds.begin(2, 'cpu', 'split', True) is None
    a, b = PairBounds.begin(2, 'cpu', 'split', True), PairBounds.begin(2, 'cpu', 'split', True)
    assert a.t.data_ptr() != b.t.data_ptr()                                 # one per forward


@pytest.mark.parametrize('on', [False, True])
def test_pair_dgrad_is_read_only(on):
    """``pair_dgrad`` is what the layout was built with: a model cannot be switched after its images exist."""
    cfg = workload_config('C2')
    m = OneTransModel.__new__(OneTransModel)
    torch.nn.Module.__init__(m)
    m.layout = FlatLayout(cfg, cfg.ns_input_width(), pair_dgrad=on)
    assert m.pair_dgrad is on
    assert any(o == 'dgrad' for (_, o) in m.layout.pair_images) == on
    with pytest.raises(AttributeError):
        m.pair_dgrad = not on
