#!/usr/bin/env python3
"""The masked Gaussian likelihood of sample paths: the fused kernels (snsde_sample_loglik / _backward) against the
same definition in tensor ops.  Same process, HIP events, the variants alternating; time, peak allocated memory, and the GB/s the
fused forward reaches against the bytes it must touch, (N V + 2 V) 4 per group (ys once, target and mask once).

Shapes (outer, B, W), S paths per row, about 40 % of the entries missing (NaN in the target):
  (1, 50, 200 x 41), S in {1, 10}      the interpolation benchmark's PhysioNet batch and its k_iwae range
  (2, 1024, 128), S in {8, 32, 128}    the shape of the other score files
  (100, 256, 16), S = 32               the layout of a solve: 100 output times in front
  fused     engine.sample_loglik on CUDA float32 (one launch forward, one backward)
  ops       engine.sample_loglik_tensor_ops, autograd for the backward
forward alone (no_grad, stats=True: bound, logpx, count, sqerr) and forward + backward (dL/d ys of the mean bound).

usage: python tools/time_sample_loglik.py [output file, default profiles/sample_loglik_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_loglik_ab.txt')
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


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


def fmt(v):
    v = np.array(v) * 1e3
    return f'median {np.median(v):9.1f} us  min {v.min():9.1f}  p90 {np.percentile(v, 90):9.1f}  ({len(v)} calls)'


def alternate(fns, blocks=8, per=5):
    t = {k: [] for k in fns}
    for f in fns.values():
        event_ms(f, 2)
    for _ in range(blocks):
        for k, f in fns.items():
            t[k] += event_ms(f, per)
    return t


say('# tools/time_sample_loglik.py: ys (outer, B S, W) float32, target (outer, B, W) with NaN at ~40 % of the entries, std 0.1, log_weight (B, S);')
say('# HIP events, variants alternating in one process; GB/s = (N V + 2 V) 4 bytes per group over the median time of the fused forward')
say('# the samples of unobserved entries are not loaded, so the bytes actually moved are fewer than that figure: the GB/s is an upper estimate of the achieved rate')
for O, B, W, Sn in ((1, 50, 200 * 41, 1), (1, 50, 200 * 41, 10), (2, 1024, 128, 8), (2, 1024, 128, 32), (2, 1024, 128, 128), (100, 256, 16, 32)):
    gen = torch.Generator().manual_seed(Sn)
    y = torch.randn(O, B, W, generator=gen)
    x = (y.repeat_interleave(Sn, 1) + 0.1 * torch.randn(O, B * Sn, W, generator=gen)).to(dev)
    y[torch.rand(O, B, W, generator=gen) < 0.4] = float('nan')
    y = y.to(dev)
    lw = (0.1 * torch.randn(B, Sn, generator=gen)).to(dev)
    xg = x.clone().requires_grad_(True)
    kw = dict(std=0.1, log_weight=lw)
    fwd = {'fused': lambda: S.sample_loglik(x, Sn, y, stats=True, **kw), 'ops': lambda: engine.sample_loglik_tensor_ops(x, Sn, y, stats=True, **kw)}

    def train(f):
        def run():
            xg.grad = None
            f(xg).mean().backward()
        return run
    bwd = {'fused': train(lambda a: S.sample_loglik(a, Sn, y, **kw)), 'ops': train(lambda a: engine.sample_loglik_tensor_ops(a, Sn, y, **kw))}
    V = O * W
    say(f'## (outer, B, W) = ({O}, {B}, {W}), S = {Sn}: N = {Sn}, V = {V}, {B} groups, ys {x.numel() * 4 / 2 ** 20:.1f} MiB')
    ref = engine.sample_loglik_tensor_ops(x.double(), Sn, y.double(), stats=True, std=0.1, log_weight=lw.double())
    with torch.no_grad():
        for k, f in fwd.items():
            got = f()
            say(f'{k:6s} max |bound - float64 statement| {float((got[0].double() - ref[0]).abs().max()):.3e} (|bound| ~ {float(ref[0].abs().mean()):.1f})'
                f'   max |sqerr - float64| {float((got[3].double() - ref[3]).abs().max()):.3e} (sqerr ~ {float(ref[3].mean()):.3f})')
        tf = alternate(fwd)
        mf = {k: peak_mb(f) for k, f in fwd.items()}
    tb = alternate(bwd)
    mb = {k: peak_mb(f) for k, f in bwd.items()}
    for k in fwd:
        say(f'forward            {k:6s} {fmt(tf[k])}   peak {mf[k]:9.1f} MiB')
    for k in bwd:
        say(f'forward + backward {k:6s} {fmt(tb[k])}   peak {mb[k]:9.1f} MiB')
    touched = B * (Sn * V + 2 * V) * 4
    say(f'fused forward: {touched / 2 ** 20:.1f} MiB to touch, {touched / (np.median(tf["fused"]) * 1e-3) / 1e9:.0f} GB/s at the median '
        f'({np.median(tf["ops"]) / np.median(tf["fused"]):.1f} x the tensor-op statement; forward + backward {np.median(tb["ops"]) / np.median(tb["fused"]):.1f} x)')
    del x, y, xg, ref, lw
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
