"""CPU: the float64 Adam reference the GPU tests compare against (a known answer), and the dense-optimizer
selection of the configuration (config.dense_optimizer_spec, train.py:53-76)."""

import math

import numpy as np

import adam_ref
from recommend_amd.config import OneTransConfig, dense_optimizer_spec


def test_adam_ref_known_answer():
    one = np.array([1.0])
    w, m, v = adam_ref.adam_update(one, 2.0 * one, 0.0 * one, 0.0 * one, 0.01, 0.9, 0.999, 1e-7, 1)
    assert abs(m[0] - 0.2) < 1e-12 and abs(v[0] - 0.004) < 1e-12
    # alpha = lr sqrt(0.001) / 0.1; w -= 0.2 alpha / (sqrt(0.004) + eps) = lr / (1 + eps / sqrt(0.004))
    assert abs(w[0] - (1.0 - 0.01 / (1.0 + 1e-7 / math.sqrt(0.004)))) < 1e-12
    assert abs(w[0] - 0.9900000158) < 1e-9
    # beta2 = 1 (the reference's default optimizer_config): alpha = 0, the weight does not move, m does
    w1, m1, v1 = adam_ref.adam_update(one, 2.0 * one, 0.0 * one, 0.5 * one, 0.01, 0.9, 1.0, 1e-7, 1)
    assert w1[0] == 1.0 and v1[0] == 0.5 and abs(m1[0] - 0.2) < 1e-12
    # clip_by_norm: a norm above the clip is scaled to it, one below is left, clip 0 is off, a zero vector stays
    g = np.array([3.0, 4.0])
    assert np.allclose(adam_ref.clip_by_norm(g, 2.5), [1.5, 2.0], rtol=0, atol=1e-15)
    assert np.array_equal(adam_ref.clip_by_norm(g, 50.0), g) and np.array_equal(adam_ref.clip_by_norm(g, 0.0), g)
    assert np.array_equal(adam_ref.clip_by_norm(np.zeros(3), 1.0), np.zeros(3))


def test_dense_optimizer_spec():
    cfg = OneTransConfig()
    # an untouched default config: RMSprop with the values the trainer has always used
    assert dense_optimizer_spec(cfg) == ('rmsprop', {'lr': 0.005, 'rho': 0.9, 'eps': 1e-7, 'momentum': 0.99999})
    cfg.rmsprop_rho, cfg.rmsprop_epsilon = 0.8, 1e-6
    cfg.optimizer_config = {'dense_optimizer': 'rmsprop', 'dense_lr': 0.01}
    assert dense_optimizer_spec(cfg) == ('rmsprop', {'lr': 0.01, 'rho': 0.8, 'eps': 1e-6, 'momentum': 0.0})
    # 'adam': beta1 / beta2 / epsilon of optimizer_config, else 0.9 / 0.999 / 1e-8
    cfg = OneTransConfig()
    cfg.optimizer_config = dict(cfg.optimizer_config, dense_optimizer='adam')
    assert dense_optimizer_spec(cfg) == ('adam', {'lr': 0.005, 'beta1': 0.1, 'beta2': 1.0, 'eps': 1e-8})
    cfg.optimizer_config = {'dense_optimizer': 'adam', 'dense_lr': 0.002, 'epsilon': 1e-6}
    assert dense_optimizer_spec(cfg) == ('adam', {'lr': 0.002, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-6})
    # dense_lr falls back to learning_rate; the reference's 'learning_rate' key is not read
    cfg.learning_rate = 0.0123
    cfg.optimizer_config = {'dense_optimizer': 'adam', 'learning_rate': 7.0}
    assert dense_optimizer_spec(cfg) == ('adam', {'lr': 0.0123, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-8})
    # any other name, or none: Adam with the Keras defaults (epsilon 1e-7), optimizer_config's betas not read
    for oc in ({'dense_optimizer': 'sgd', 'beta1': 0.5, 'beta2': 0.5, 'epsilon': 1.0}, {}):
        cfg.optimizer_config = oc
        assert dense_optimizer_spec(cfg) == ('adam', {'lr': 0.0123, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-7})
    # no new config attribute: a round trip through to_dict / from_dict gives the same spec
    cfg = OneTransConfig()
    assert dense_optimizer_spec(OneTransConfig.from_dict(cfg.to_dict())) == dense_optimizer_spec(cfg)
