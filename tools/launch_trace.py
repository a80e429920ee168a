"""Launch lists and result hashes of the transformer block over a fixed list of cases that between them reach every
gate of the block's forward and backward (which launch runs, with which side outputs).  For comparing two trees that
must launch the same kernels and compute the same bits:

    python tools/launch_trace.py --out a.json          (on one tree)
    python tools/launch_trace.py --out b.json          (on the other)
    python tools/launch_trace.py --compare a.json b.json

Each case builds a small model (C2 cut to 2 layers, 12 NS tokens, three sequences of 20, ffn_dim = 2 d, B = 37, fixed
init), runs one training forward, the loss and the backward, then one ``torch.no_grad()`` forward, all under a probe,
and records the launch list ('--' separates the two phases), the sha256 of the training probabilities, of the flat
gradient buffer and of the no-grad probabilities.  Uses only the public model surface (OneTransModel, keras_bce_loss,
K.Probe / K.set_probe and the switches in kernels.py), so it runs on older checkouts too."""

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from recommend_amd import kernels as K  # noqa: E402
from recommend_amd.config import workload_config  # noqa: E402
from recommend_amd.data import make_batch, ragged_lengths  # noqa: E402
from recommend_amd.model import OneTransModel, keras_bce_loss  # noqa: E402
from recommend_amd.params import init_params  # noqa: E402
from recommend_amd.trainer import stack_labels  # noqa: E402

B = 37
PYRAMID = dict(pyramid_enabled=True, pyramid_ratios=[0.5, 0.25], dedicated_positions='tail')

# name -> dict(d, H, dropout, mode ('split' | 'f32' | 'bf16' | 'fp8attn'), cfg (config attributes), env, model (model
# attributes set after construction), last_fold, ragged)
CASES = {
    'split_d128_drop0': dict(dropout=0.0),
    'split_d128': dict(),
    'split_d128_pair_dgrad_off': dict(env={'ONETRANS_PAIR_DGRAD': '0'}),
    'split_d128_pair_wgrad_off': dict(env={'ONETRANS_PAIR_WGRAD': '0'}),
    'split_d128_recompute': dict(cfg=dict(recompute_blocks=True)),
    'split_d128_fuse_bwd_off': dict(model=dict(fuse_bwd=False)),
    'split_d128_accumulate': dict(model=dict(accumulate_grads=True)),
    'split_d128_padding_mask': dict(cfg=dict(seq_padding_mask=True), ragged=True),
    'split_d128_pyramid_tail': dict(cfg=dict(pyramid_select='tail', **PYRAMID)),
    'split_d128_pyramid_norm': dict(cfg=dict(pyramid_select='norm', **PYRAMID)),
    'split_d128_last_fold0': dict(last_fold=0),
    'split_d128_last_fold1': dict(last_fold=1),
    'split_d64': dict(d=64),
    'split_d256': dict(d=256),
    'split_d384': dict(d=384, H=6),
    'f32_d128': dict(mode='f32'),
    'bf16_d128': dict(mode='bf16'),
    'bf16_d256': dict(mode='bf16', d=256),
    'fp8attn_d256': dict(mode='fp8attn', d=256),
}


def model_cfg(d=128, H=4, dropout=0.1, **kw):
    cfg = workload_config('C2')
    cfg.hidden_dim, cfg.num_heads, cfg.ffn_dim, cfg.num_layers, cfg.num_ns_tokens = d, H, 2 * d, 2, 12
    cfg.sparse_features = {k: 40 + 7 * i for i, k in enumerate(cfg.sparse_features)}
    cfg.seq_item_vocab = 300
    cfg._seq_lens = [20, 20, 20]
    cfg.dropout_rate = dropout
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def to_dev(dct, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dct.items()}


def run_case(case, dev):
    mode = case.get('mode', 'split')
    env = case.get('env', {})
    old_env = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    old_mode = K.set_matmul_mode('bf16' if mode in ('bf16', 'fp8attn') else mode)   # as bench.py --precision
    old_fold = K.last_fold()
    try:
        cfg = model_cfg(case.get('d', 128), case.get('H', 4), case.get('dropout', 0.1), **case.get('cfg', {}))
        cfg.compute_dtype = {'fp8attn': 'fp8attn', 'bf16': 'bf16'}.get(mode, 'fp32')
        if 'last_fold' in case:
            K.last_fold(case['last_fold'])
        P = init_params(cfg, cfg.ns_input_width(), seed=0, perturb=True)
        ns, seq, lab = make_batch(B, cfg, seed=1000)
        if case.get('ragged'):
            seq = {**seq, **ragged_lengths(B, cfg, seed=11)}
        model = OneTransModel(cfg, device=dev, init=P)
        for k, v in case.get('model', {}).items():
            setattr(model, k, v)
        model.flat.grad.fill_(1.0 if model.accumulate_grads else float('nan'))
        ns_d, seq_d = to_dev(ns, dev), to_dev(seq, dev)
        probe = K.Probe()
        K.set_probe(probe)
        probs = model.forward_probs(ns_d, seq_d, training=True)
        keras_bce_loss(stack_labels(lab, cfg.tasks, dev), probs, cfg.tasks).backward()
        torch.cuda.synchronize()
        n_train = len(probe.recs)
        with torch.no_grad():
            eval_probs = model.forward_probs(ns_d, seq_d, training=False)
        torch.cuda.synchronize()
        K.set_probe(None)
        launches = [f'{r[0]} {r[4]}' for r in probe.recs]
        return dict(launches=launches[:n_train] + ['--'] + launches[n_train:], probs_sha256=sha(probs),
                    grad_sha256=sha(model.flat.grad), eval_probs_sha256=sha(eval_probs))
    finally:
        K.set_probe(None)
        K.set_matmul_mode(old_mode)
        K.last_fold(old_fold)
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def compare(path_a, path_b) -> int:
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f'{name}: only in {path_a if name in a else path_b}')
            bad += 1
            continue
        diff = [k for k in a[name] if a[name][k] != b[name].get(k)]
        n = len(a[name]['launches']) - 1
        print(f'{name}: {n} launches, ' + ('equal' if not diff else 'DIFFER in ' + ', '.join(diff)))
        if 'launches' in diff:
            for i, (x, y) in enumerate(zip(a[name]['launches'], b[name]['launches'])):
                if x != y:
                    print(f'    first difference at launch {i}: {x!r} / {y!r}')
                    break
        bad += bool(diff)
    print(f'{len(a)} cases, {bad} differ')
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', help='write the trace of every case to this JSON file')
    ap.add_argument('--cases', nargs='*', default=list(CASES), help='case names (default: all)')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'),
                    help='compare two trace files; exit status 1 if they differ')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    out = {}
    for name in args.cases:
        out[name] = run_case(CASES[name], 'cuda:0')
        print(f"{name}: {len(out[name]['launches']) - 1} launches  probs {out[name]['probs_sha256'][:12]}  "
              f"grad {out[name]['grad_sha256'][:12]}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
