"""CPU: multi-valued NS features (``OneTransConfig.bag_features``) — configuration, table layout, input helpers and
the float64 yardstick tests/bag_ref.py against torch.nn.functional.embedding_bag."""

import json

import numpy as np
import pytest
import torch

import bag_ref as BR
from recommend_amd.config import OneTransConfig, check_bag_features, workload_config
from recommend_amd.data import criteo_batch, expand_requests, make_batch, make_request_batch
from recommend_amd.features import FeatureProcessor
from recommend_amd.params import init_tables, ns_table_offsets


def bag_config():
    """C2 scaled down, with three bag features placed among the single-id and dense features."""
    cfg = workload_config('C2')
    cfg.sparse_features = {k: 40 + 7 * i for i, k in enumerate(cfg.sparse_features)}
    cfg.seq_item_vocab = 300
    fc = cfg.feature_config
    fc['user_features'] = ['tags'] + fc['user_features']                  # before every single-id feature
    fc['item_features'] = fc['item_features'][:3] + ['cats'] + fc['item_features'][3:]
    fc['context_features'] = fc['context_features'][:2] + ['sim_items'] + fc['context_features'][2:]
    cfg.bag_features = {'tags': {'cardinality': 23, 'pooling': 'sum'},
                        'cats': {'cardinality': 11},
                        'sim_items': {'table': 'seq_item', 'pooling': 'mean'}}
    return cfg


def test_config_round_trip_and_default():
    assert OneTransConfig().bag_features == {}
    cfg = bag_config()
    d = json.loads(json.dumps(cfg.to_dict()))
    back = OneTransConfig.from_dict(d)
    assert back.bag_features == cfg.bag_features
    back.bag_features['tags']['pooling'] = 'mean'
    assert cfg.bag_features['tags']['pooling'] == 'sum'                   # a deep copy
    check_bag_features(back)
    assert cfg.bag_pooling('cats') == 'mean'                              # the default pooling
    assert cfg.bag_rows('sim_items') == 300 and cfg.bag_rows('tags') == 23


@pytest.mark.parametrize('edit,match', [
    (lambda c: c.sparse_features.update(tags=5), 'also in sparse_features'),
    (lambda c: c.bag_features['tags'].update(pooling='max'), 'unknown pooling'),
    (lambda c: c.bag_features.update(sim_items={'table': 'seq_user'}), 'unknown table'),
    (lambda c: c.bag_features.update(ghost={'cardinality': 4}), 'none of the user / item / context'),
    (lambda c: setattr(c, 'seq_item_vocab', 0), 'needs seq_item_vocab'),
    (lambda c: c.bag_features.update(cats={'pooling': 'sum'}), "positive 'cardinality'"),
])
def test_check_bag_features_errors(edit, match):
    cfg = bag_config()
    check_bag_features(cfg)
    edit(cfg)
    with pytest.raises(ValueError, match=match):
        check_bag_features(cfg)


def test_widths_and_offsets():
    plain = workload_config('C2')
    plain.sparse_features = {k: 40 + 7 * i for i, k in enumerate(plain.sparse_features)}
    cfg = bag_config()
    e, E = cfg.ns_embedding_dim, cfg.seq_feature_dim
    assert plain.ns_input_width() == 13 + 26 * e
    assert cfg.ns_input_width() == plain.ns_input_width() + 2 * e + E
    assert cfg.ns_input_width(['tags', 'C1', 'I1', 'sim_items']) == e + e + 1 + E
    # without bag features: exactly the running sum of the single-id cardinalities, as before
    offs, run = ns_table_offsets(plain), 0
    for n in plain.ns_feature_names():
        if n in plain.sparse_features:
            assert offs[n] == run
            run += plain.sparse_features[n]
    assert offs['__total__'] == run and set(offs) == set(plain.sparse_features) | {'__total__'}
    # with them: one running sum over ns_feature_names(); a 'seq_item' bag owns no rows of emb.ns
    offs, run = ns_table_offsets(cfg), 0
    for n in cfg.ns_feature_names():
        if n in cfg.sparse_features or n in ('tags', 'cats'):
            assert offs[n] == run, n
            run += cfg.sparse_features.get(n) or cfg.bag_features[n]['cardinality']
    assert 'sim_items' not in offs and offs['__total__'] == run == sum(cfg.sparse_features.values()) + 23 + 11
    assert offs['tags'] == 0 and offs['C1'] == 23
    assert init_tables(cfg, 1)['emb.ns'].shape == (run, e)
    assert np.array_equal(init_tables(plain, 1)['emb.ns'],
                          init_tables(workload_small_plain(), 1)['emb.ns'])


def workload_small_plain():
    cfg = workload_config('C2')
    cfg.sparse_features = {k: 40 + 7 * i for i, k in enumerate(cfg.sparse_features)}
    return cfg


def test_pad_bags():
    out = FeatureProcessor.pad_bags([[3, 1, 4], [], [5]])
    assert out.dtype == np.int64 and out.tolist() == [[3, 1, 4], [-1, -1, -1], [5, -1, -1]]
    assert FeatureProcessor.pad_bags([[3, 1, 4, 1, 5], [9]], cap=3).tolist() == [[4, 1, 5], [9, -1, -1]]   # the tail
    assert FeatureProcessor.pad_bags([[], []]).shape == (2, 1)
    assert FeatureProcessor.pad_bags([[1]], cap=4).tolist() == [[1, -1, -1, -1]]
    with pytest.raises(ValueError):
        FeatureProcessor.pad_bags([[1]], cap=0)


def test_generator_and_request_carry_through():
    cfg = bag_config()
    cfg._seq_lens = [5, 9, 7]
    ns, seq, lab = make_batch(64, cfg, seed=1000)
    assert ns['tags'].shape == ns['cats'].shape == ns['sim_items'].shape == (64, 8) and ns['tags'].dtype == np.int64
    for n in cfg.bag_features:
        ids = ns[n]
        lens = (ids >= 0).sum(axis=1)
        assert lens[0] == 0 and lens[1] == 8 and len(set(lens.tolist())) > 3          # empty, full, varying
        assert ids.max() < cfg.bag_rows(n) and ids.min() == -1
        assert np.all((ids >= 0) == (np.arange(8)[None] < lens[:, None]))             # left-packed
    assert ns['tags_weight'].shape == (64, 8) and ns['tags_weight'].dtype == np.float32
    assert 'cats_weight' not in ns and 'sim_items_weight' not in ns                   # 'mean' bags take no weights
    # every other array of the batch is what the config without bag features draws
    plain = bag_config()
    plain._seq_lens = [5, 9, 7]
    for group in ('user_features', 'item_features', 'context_features'):
        plain.feature_config[group] = [n for n in plain.feature_config[group] if n not in plain.bag_features]
    plain.bag_features = {}
    ns0, seq0, lab0 = make_batch(64, plain, seed=1000)
    assert all(np.array_equal(ns[k], v) for k, v in ns0.items())
    assert all(np.array_equal(seq[k], v) for k, v in seq0.items())
    assert all(np.array_equal(lab[k], v) for k, v in lab0.items())
    # explicit caps and fills
    ns2, _, _ = criteo_batch(32, cfg, seed=3, bags={'tags': 3, 'sim_items': (16, 4.0)})
    assert ns2['tags'].shape == (32, 3) and ns2['sim_items'].shape == (32, 16) and 'cats' not in ns2
    # request-grouped batches carry the candidates' bags, and expansion leaves them alone
    rb = make_request_batch(3, [2, 0, 4], cfg, seed=7)
    assert rb[0]['sim_items'].shape == (6, 8) and rb[1]['click_seq'].shape[0] == 3
    ens, eseq, _ = expand_requests(rb)
    assert ens['sim_items'] is rb[0]['sim_items'] and eseq['click_seq'].shape[0] == 6


def ragged(ids, weights, num_rows):
    """The padded form as embedding_bag's (input, offsets, per_sample_weights)."""
    ok = BR.valid(ids, num_rows)
    lens = ok.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    w = None if weights is None else torch.from_numpy(weights[ok].astype(np.float64))
    return torch.from_numpy(ids[ok]), torch.from_numpy(offsets), w


@pytest.mark.parametrize('pooling,weighted', [('sum', False), ('sum', True), ('mean', False)])
def test_bag_ref_pool_matches_embedding_bag(pooling, weighted):
    rng = np.random.default_rng(5)
    rows, E, B, cap, off = 19, 8, 33, 7, 4
    table = rng.normal(size=(off + rows + 3, E))
    ids = rng.integers(0, rows, size=(B, cap))
    ids[rng.random((B, cap)) < 0.4] = -1
    ids[0] = -1                                             # an empty bag
    ids[1] = 5                                              # one id repeated in a full bag
    ids[2, :3] = [0, rows - 1, rows]                        # first row, last row, one past the end (an empty slot)
    ids[3, 0] = rows + 100
    w = rng.uniform(0.25, 2.0, size=(B, cap)).astype(np.float32) if weighted else None
    got = BR.pool(table, ids, w, pooling, off, rows)
    inp, offsets, psw = ragged(ids, w, rows)
    want = torch.nn.functional.embedding_bag(inp + off, torch.from_numpy(table), offsets, mode=pooling,
                                             per_sample_weights=psw).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    assert np.all(got[0] == 0)
    c = BR.coefs(ids, w, pooling, rows)
    assert c.dtype == np.float32 and np.all(c[~BR.valid(ids, rows)] == 0)
    table32 = table.astype(np.float32).astype(np.float64)
    via_coef = (table32[off + np.where(BR.valid(ids, rows), ids, 0)] * c.astype(np.float64)[:, :, None]).sum(axis=1)
    np.testing.assert_allclose(via_coef, BR.pool(table32, ids, w, pooling, off, rows), rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        BR.pool(table, ids, np.ones(ids.shape), 'mean', off, rows)


def test_tokenizer_bags_places_the_columns(monkeypatch):
    """The patched oracle tokenizer equals a hand-built NS concat, and its table gradient reaches the bag rows."""
    from oracle import onetrans_ref as R
    from recommend_amd.params import init_params
    cfg = bag_config()
    cfg.hidden_dim, cfg.num_heads, cfg.ffn_dim, cfg.num_layers, cfg.num_ns_tokens = 16, 2, 32, 1, 2
    cfg._seq_lens = [2, 2, 2]
    P = R.to_torch(init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True))
    ns, seq, _ = make_batch(6, cfg, seed=11)
    offs = ns_table_offsets(cfg)
    parts = []
    for n in cfg.ns_feature_names():
        if n in cfg.bag_features:
            t = 'emb.seq_item' if n == 'sim_items' else 'emb.ns'
            parts.append(BR.pool(P[t].numpy(), ns[n], ns.get(n + '_weight'), cfg.bag_pooling(n), offs.get(n, 0),
                                 cfg.bag_rows(n)))
        elif n in cfg.sparse_features:
            parts.append(P['emb.ns'].numpy()[offs[n] + ns[n][:, 0]])
        else:
            parts.append(ns[n].astype(np.float64))
    nsmat = np.concatenate(parts, axis=1)
    assert nsmat.shape[1] == cfg.ns_input_width()
    want = (nsmat @ P['tok.ns.kernel'].numpy() + P['tok.ns.bias'].numpy()).reshape(6, cfg.num_ns_tokens, -1)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x = BR.tokenizer_bags(leaves, cfg, R.to_torch(ns), R.to_torch(seq))
    np.testing.assert_allclose(x[:, -cfg.num_ns_tokens:].detach().numpy(), want, rtol=0, atol=1e-12)
    x.sum().backward()
    g = leaves['emb.ns'].grad
    used = np.unique(ns['tags'][ns['tags'] >= 0]) + offs['tags']
    assert torch.all(g[used].abs().sum(dim=1) > 0)
    unused = np.setdiff1d(np.arange(offs['tags'], offs['tags'] + 23), used)
    assert torch.all(g[unused] == 0)


def test_optimizer_joins_the_entries_of_one_table():
    """OneTransOptimizer._join_pending: entries naming one table become one (keys, grads) in order; a list without
    repeated names is returned as it is (the same tensors, today's path)."""
    from recommend_amd.trainer import OneTransOptimizer
    k = [torch.tensor([3, -1, 5]), torch.tensor([[1, 2], [3, 4]]), torch.tensor([7])]
    g = [torch.ones(3, 4), torch.full((4, 4), 2.0), torch.full((1, 8), 3.0)]
    single = [('emb.ns', k[0], g[0]), ('emb.seq_item', k[2], g[2])]
    assert OneTransOptimizer._join_pending(single) is single
    out = OneTransOptimizer._join_pending([('emb.ns', k[0], g[0]), ('emb.seq_item', k[2], g[2]),
                                           ('emb.ns', k[1], g[1])])
    assert [n for n, _, _ in out] == ['emb.ns', 'emb.seq_item']
    assert out[0][1].tolist() == [3, -1, 5, 1, 2, 3, 4] and out[0][2].shape == (7, 4)
    assert torch.equal(out[0][2][3:], g[1]) and out[1][1] is k[2] and out[1][2] is g[2]


def test_descriptor_layout_and_limits_match_the_header():
    import ctypes
    import re
    from recommend_amd import _lib
    txt = open(_lib.HEADER).read()
    defs = dict(re.findall(r'#define (OT_(?:NS_BAG|BAG)_[A-Z_]+) (\d+)', txt))
    assert int(defs['OT_NS_BAG_MAX']) == _lib.NS_BAG_MAX and int(defs['OT_NS_BAG_MAX_WIDTH']) == _lib.NS_BAG_MAX_WIDTH
    assert _lib.BAG_POOLINGS == {'sum': int(defs['OT_BAG_SUM']), 'mean': int(defs['OT_BAG_MEAN'])}
    body = re.search(r'typedef struct \{([^}]*)\} ot_ns_bag;', txt).group(1)
    names = re.findall(r'(\w+);', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert names == [f[0] for f in _lib.NsBag._fields_]
    assert ctypes.sizeof(_lib.NsBag) == 7 * 8 + 4 * 4 and _lib.NsBag.width.offset == 56
