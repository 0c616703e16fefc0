#!/usr/bin/env python3
"""Scores of sample paths: the fused kernels (snsde_sample_crps / _backward, snsde_sample_quantiles) against the
same definitions in tensor ops.  Same process, HIP events, the variants alternating; time and peak allocated memory.

At (T, B, S, H) = (2, 1024, S, 128), S in {8, 32, 128} - the result of a K2-architecture solve with S paths per row:
  fused     engine.sample_crps on CUDA float32 (one launch forward, one backward)
  sort      engine.sample_crps_tensor_ops: the counts from a sort of each column, autograd for the backward
  pairwise  mean |x - y| - sum_ij |x_i - x_j| / (2 S (S - 1)) with the (T, B, S, S, H) differences (where they stay under 4 GiB)
forward alone (no_grad) and forward + backward (dL/d ys and dL/d target of the mean score).  Then five quantile levels, forward:
engine.sample_quantiles against torch.quantile.

usage: python tools/time_sample_scores.py [output file, default profiles/sample_scores_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_scores_ab.txt')
lines = []
T, B, H = 2, 1024, 128
QS = (0.05, 0.25, 0.5, 0.75, 0.95)


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


def alternate(fns, blocks=10, per=10):
    t = {k: [] for k in fns}
    for f in fns.values():
        event_ms(f, 3)
    for _ in range(blocks):
        for k, f in fns.items():
            t[k] += event_ms(f, per)
    return t


def pairwise(x, y, Sn):
    v = x.reshape(T, B, Sn, H)
    return (v - y.unsqueeze(-2)).abs().mean(-2) - (v.unsqueeze(-2) - v.unsqueeze(-3)).abs().sum((-2, -3)) / (2 * Sn * (Sn - 1))


say(f'# tools/time_sample_scores.py: ys (T, B S, H) = ({T}, {B} S, {H}) float32, target ({T}, {B}, {H}); HIP events, variants alternating')
say('# peak = the most allocated during one call above what was allocated when it began; a forward + backward call begins with the previous')
say("# call's gradients (1 x ys + 1 x target) still allocated and frees them first, so its own gradients are not in its figure - for every variant alike")
for Sn in (8, 32, 128):
    gen = torch.Generator().manual_seed(Sn)
    x = torch.randn(T, B * Sn, H, generator=gen).to(dev)
    y = torch.randn(T, B, H, generator=gen).to(dev)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    fwd = {'fused': lambda: S.sample_crps(x, Sn, y), 'sort': lambda: engine.sample_crps_tensor_ops(x, Sn, y)}
    if T * B * Sn * Sn * H * 4 < 4 * 2 ** 30:
        fwd['pairwise'] = lambda: pairwise(x, y, Sn)

    def train(f):
        def run():
            xg.grad = yg.grad = None
            f(xg, yg).mean().backward()
        return run
    bwd = {'fused': train(lambda a, b: S.sample_crps(a, Sn, b)), 'sort': train(lambda a, b: engine.sample_crps_tensor_ops(a, Sn, b))}
    if 'pairwise' in fwd:
        bwd['pairwise'] = train(lambda a, b: pairwise(a, b, Sn))
    say(f'## S = {Sn}: ys {x.numel() * 4 / 2 ** 20:.0f} MiB')
    ref = engine.sample_crps_tensor_ops(x.double(), Sn, y.double())
    with torch.no_grad():
        for k, f in fwd.items():
            say(f'{k:9s} max |crps - float64 sort statement| {float((f().double() - ref).abs().max()):.3e}')
        tf = alternate(fwd)
        mf = {k: peak_mb(f) for k, f in fwd.items()}
    tb = alternate(bwd)
    mb = {k: peak_mb(f) for k, f in bwd.items()}
    for k in fwd:
        say(f'forward            {k:9s} {fmt(tf[k])}   peak {mf[k]:9.1f} MiB')
    for k in bwd:
        say(f'forward + backward {k:9s} {fmt(tb[k])}   peak {mb[k]:9.1f} MiB')
    with torch.no_grad():
        qf = {'fused': lambda: S.sample_quantiles(x, Sn, QS),
              'torch.quantile': lambda: torch.quantile(x.reshape(T, B, Sn, H), torch.tensor(QS, device=dev), dim=2)}
        say(f'quantiles max |fused - torch.quantile| {float((qf["fused"]() - qf["torch.quantile"]()).abs().max()):.3e}')
        tq = alternate(qf)
        for k, f in qf.items():
            say(f'quantiles {QS}  {k:15s} {fmt(tq[k])}   peak {peak_mb(f):9.1f} MiB')
    del x, y, xg, yg, ref
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
