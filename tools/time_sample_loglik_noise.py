#!/usr/bin/env python3
"""sample_loglik under a tensor noise: the noise kernels (snsde_sample_loglik_noise / _backward / _reduce) in
per-channel and per-entry mode against the scalar kernel (snsde_sample_loglik, the baseline: unchanged code) and against the
tensor-op statement with a tensor log_std.  Same process, HIP events, the variants alternating in blocks of five with a rotating starting variant, medians of 40 calls.

Shapes (outer, B, W), S paths per row, about 40 % of the entries missing - those of profiles/sample_loglik_ab.txt:
  (1, 50, 200 x 41), S in {1, 10}; (2, 1024, 128), S in {8, 32, 128}; (100, 256, 16), S = 32.
  scalar    engine.sample_loglik(std=0.1)
  channel   engine.sample_loglik(log_std=(W,))            backward: one launch + the reduce
  entry     engine.sample_loglik(log_std=(outer, B, W))   backward: one launch
  ops       engine.sample_loglik_tensor_ops(log_std=(W,)), autograd for the backward
forward alone (no_grad, stats=True) and forward + backward (dL/d ys of the mean bound, and dL/d log_std where there is one).
Each variant is reported as a ratio to the scalar kernel, beside the ratio of the bytes each must touch: the scalar forward
(N V + 2 V) 4 per group, entry mode one (V) plane more - 1 / (N + 2) of it - and channel mode W floats in all.

usage: python tools/time_sample_loglik_noise.py [output file, default profiles/sample_loglik_noise_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_loglik_noise_ab.txt')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def event_ms(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def fmt(v):
    v = np.array(v) * 1e3
    return f'median {np.median(v):9.1f} us  min {v.min():9.1f}  p90 {np.percentile(v, 90):9.1f}  ({len(v)} calls)'


def alternate(fns, blocks=8, per=5):
    t = {k: [] for k in fns}
    for f in fns.values():
        event_ms(f, 2)
    keys = list(fns)
    for b in range(blocks):      # (the starting variant rotates from block to block: no variant is always the first after a pause)
        for k in keys[b % len(keys):] + keys[:b % len(keys)]:
            t[k] += event_ms(fns[k], per)
    return t


say('# tools/time_sample_loglik_noise.py: ys (outer, B S, W) float32, target (outer, B, W) with NaN at ~40 % of the entries, log_weight (B, S);')
say('# scalar: std = 0.1; channel: log_std (W,); entry: log_std (outer, B, W); ops: the tensor-op statement with the (W,) log_std')
say('# HIP events, variants alternating in one process (eight blocks of five, the starting variant rotating), medians of 40; "x scalar" = median over the scalar kernel\'s median')
for O, B, W, Sn in ((1, 50, 200 * 41, 1), (1, 50, 200 * 41, 10), (2, 1024, 128, 8), (2, 1024, 128, 32), (2, 1024, 128, 128), (100, 256, 16, 32)):
    gen = torch.Generator().manual_seed(Sn)
    y = torch.randn(O, B, W, generator=gen)
    x = (y.repeat_interleave(Sn, 1) + 0.1 * torch.randn(O, B * Sn, W, generator=gen)).to(dev)
    y[torch.rand(O, B, W, generator=gen) < 0.4] = float('nan')
    y = y.to(dev)
    lw = (0.1 * torch.randn(B, Sn, generator=gen)).to(dev)
    lc = (0.2 * torch.randn(W, generator=gen) + float(np.log(0.1))).to(dev)
    le = lc.expand(O, B, W).contiguous()
    xg, lcg, leg = x.clone().requires_grad_(True), lc.clone().requires_grad_(True), le.clone().requires_grad_(True)
    fwd = {'scalar': lambda: S.sample_loglik(x, Sn, y, std=0.1, log_weight=lw, stats=True),
           'channel': lambda: S.sample_loglik(x, Sn, y, log_std=lc, log_weight=lw, stats=True),
           'entry': lambda: S.sample_loglik(x, Sn, y, log_std=le, log_weight=lw, stats=True),
           'ops': lambda: engine.sample_loglik_tensor_ops(x, Sn, y, log_std=lc, log_weight=lw, stats=True)}

    def train(f, *leaves):
        def run():
            for t in leaves:
                t.grad = None
            f().mean().backward()
        return run
    bwd = {'scalar': train(lambda: S.sample_loglik(xg, Sn, y, std=0.1, log_weight=lw), xg),
           'channel': train(lambda: S.sample_loglik(xg, Sn, y, log_std=lcg, log_weight=lw), xg, lcg),
           'entry': train(lambda: S.sample_loglik(xg, Sn, y, log_std=leg, log_weight=lw), xg, leg),
           'ops': train(lambda: engine.sample_loglik_tensor_ops(xg, Sn, y, log_std=lcg, log_weight=lw), xg, lcg)}
    V = O * W
    say(f'## (outer, B, W) = ({O}, {B}, {W}), S = {Sn}: N = {Sn}, V = {V}, {B} groups, ys {x.numel() * 4 / 2 ** 20:.1f} MiB')
    ref = engine.sample_loglik_tensor_ops(x.double(), Sn, y.double(), stats=True, log_std=lc.double(), log_weight=lw.double())
    with torch.no_grad():
        for k in ('channel', 'entry', 'ops'):
            got = fwd[k]()
            say(f'{k:8s} max |bound - float64 statement| {float((got[0].double() - ref[0]).abs().max()):.3e} (|bound| ~ {float(ref[0].abs().mean()):.1f})')
        tf = alternate(fwd)
    tb = alternate(bwd)
    base_f, base_b = np.median(tf['scalar']), np.median(tb['scalar'])
    for k in fwd:
        say(f'forward            {k:8s} {fmt(tf[k])}   {np.median(tf[k]) / base_f:5.2f} x scalar')
    for k in bwd:
        say(f'forward + backward {k:8s} {fmt(tb[k])}   {np.median(tb[k]) / base_b:5.2f} x scalar')
    say(f'bytes to touch, forward: entry / scalar = {(Sn * V + 3 * V) / (Sn * V + 2 * V):.3f}, channel / scalar = '
        f'{(B * (Sn * V + 2 * V) + W) / (B * (Sn * V + 2 * V)):.6f}; the tensor-op statement takes '
        f'{np.median(tf["ops"]) / np.median(tf["channel"]):.1f} x (forward) and {np.median(tb["ops"]) / np.median(tb["channel"]):.1f} x '
        f'(forward + backward) the time of the channel kernels, {np.median(tf["ops"]) / np.median(tf["entry"]):.1f} x and '
        f'{np.median(tb["ops"]) / np.median(tb["entry"]):.1f} x that of the entry kernels')
    del x, y, xg, ref, lw, lc, le, lcg, leg
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
