"""The cost of the key-padding mask, written as a markdown report.

1. Per-launch time of the masked attention (ot_attn_fwd_masked / ot_attn_bwd_masked: the generic f32 family) against the
   un-masked calls (split mode: the slice kernels) at a C2 layer (B 4096, H 4, I = K = 140, head_dim 32) and a T layer
   (head_dim 64), forward and backward.  HIP events, interleaved rounds, min / median.
2. Step time of a C2-shaped model (trainer.train_step) with ``seq_padding_mask`` on at mean fill 0.5 against the same
   model with it off, on the same batches.

`--out FILE` (default profiles/r09/padding_mask.md) receives every number measured.  Iteration tool; never part of the
product path."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from recommend_amd import kernels as K
from recommend_amd.config import workload_config
from recommend_amd.data import make_batch, ragged_lengths
from recommend_amd.trainer import OneTransTrainer

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--batch', type=int, default=4096)
ap.add_argument('--steps', type=int, default=12, help='timed training steps per variant (after 3 warm-up steps)')
ap.add_argument('--fill', type=float, default=0.5)
ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              'profiles', 'r09', 'padding_mask.md'))
args = ap.parse_args()

dev = torch.device('cuda')
K.set_matmul_mode('split')
lines = ['# Key-padding mask: measurements (tools/padmask_bench.py)', '',
         f'MI355X; split mode; HIP events; {args.rounds} interleaved rounds.', '']


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


# ---- 1. attention launches
lines += ['## 1. Attention launches, masked against un-masked', '',
          f'B {args.batch}, H 4, I = K = 140; validity: binomial lengths at mean fill {args.fill} in three segments of 42 '
          '(the C2 layout).', '',
          '| layer | pass | un-masked min / median (us) | masked min / median (us) | masked / un-masked (median) |',
          '|---|---|---|---|---|']
B, H, I = args.batch, 4, 140
rng = np.random.default_rng(0)
valid = np.ones((B, I), np.uint8)
for s in range(3):
    ln = rng.binomial(42, args.fill, size=B)
    valid[:, 43 * s:43 * s + 42] = np.arange(42)[None, :] >= 42 - ln[:, None]
kv = (torch.from_numpy(valid).to(dev), 0, I)
for name, hd in (('C2 (head_dim 32)', 32), ('T (head_dim 64)', 64)):
    d = H * hd
    qkv = torch.randn(B * I, 3 * d, device=dev)
    out, lse = torch.empty(B * I, d, device=dev), torch.empty(B * H * I, device=dev)
    dout, dqkv = torch.randn(B * I, d, device=dev), torch.empty(B * I, 3 * d, device=dev)
    K.attn_fwd_masked(qkv, 3 * d, B, H, I, I, hd, out, lse, kv)
    out_m, lse_m = out.clone(), lse.clone()
    K.attn_fwd(qkv, 3 * d, B, H, I, I, hd, out, lse)
    out_u, lse_u = out.clone(), lse.clone()
    v = {'fwd': (lambda: K.attn_fwd(qkv, 3 * d, B, H, I, I, hd, out, lse),
                 lambda: K.attn_fwd_masked(qkv, 3 * d, B, H, I, I, hd, out, lse, kv)),
         'bwd': (lambda: K.attn_bwd(qkv, 3 * d, out_u, dout, lse_u, B, H, I, I, hd, dqkv),
                 lambda: K.attn_bwd_masked(qkv, 3 * d, out_m, dout, lse_m, B, H, I, I, hd, dqkv, kv))}
    for p, (un, ma) in v.items():
        for fn in (un, ma):
            fn(); fn()
        torch.cuda.synchronize()
        tu, tm = [], []
        for _ in range(args.rounds):
            tu.append(timed(un)); tm.append(timed(ma))
        lines.append(f'| {name} | {p} | {min(tu):.1f} / {np.median(tu):.1f} | {min(tm):.1f} / {np.median(tm):.1f} | '
                     f'{np.median(tm) / np.median(tu):.2f} |')
    del qkv, out, lse, dout, dqkv, out_m, lse_m, out_u, lse_u

# ---- 2. training step of a C2-shaped model, switch on against off
lines += ['', '## 2. C2 training step, switch on against off', '',
          f'workload_config(\'C2\'), B {args.batch}, {args.steps} timed steps after 3 warm-up steps, four resident batches; '
          f'lengths: data.ragged_lengths at mean fill {args.fill}.', '',
          '| seq_padding_mask | ms / step min | ms / step median |', '|---|---|---|']
res = {}
for on in (False, True):
    cfg = workload_config('C2')
    cfg.seq_padding_mask = on
    tr = OneTransTrainer(cfg, device=dev)
    batches = []
    for i in range(4):
        ns, seq, lab = make_batch(args.batch, cfg, seed=1000 + i)
        if on:
            seq.update(ragged_lengths(args.batch, cfg, seed=i, mean_fill=args.fill))
        t = lambda dct: {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in dct.items()}
        batches.append((t(ns), t(seq), t(lab)))
    ts = []
    for i in range(3 + args.steps):
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); tr.train_step(batches[i % 4]); e1.record(); torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    res[on] = ts
    lines.append(f'| {"on" if on else "off"} | {min(ts):.2f} | {np.median(ts):.2f} |')
    del tr, batches
    torch.cuda.empty_cache()
lines += ['', f'on / off (median): {np.median(res[True]) / np.median(res[False]):.3f}', '']

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines))
print('\n'.join(lines))
