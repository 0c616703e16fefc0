#!/usr/bin/env python3
"""The energy score of sample paths: the fused kernels (snsde_sample_energy / _backward) against the same definition
in tensor ops.  Same process, HIP events, the variants alternating; time and peak allocated memory.

At (T, B, S, W) = (2, 1024, S, 128), S in {8, 32, 128} - the result of a K2-architecture solve with S paths per row, one score
per (time, row) - and path=True at (T, B, S, W) = (100, 256, 32, 16), one score per row over the whole path (V = 1600):
  fused     engine.sample_energy on CUDA float32 (one launch forward, one backward)
  cdist     engine.sample_energy_tensor_ops: vector_norm + torch.cdist in its direct-difference mode, autograd for the backward
  pairwise  the (.., N, N, V) differences written out (where they stay under 4 GiB)
forward alone (no_grad) and forward + backward (dL/d ys and dL/d target of the mean score).

usage: python tools/time_sample_energy.py [output file, default profiles/sample_energy_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_energy_ab.txt')
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


def pairwise(x, y, Sn, path):
    """The definition over the (.., N, N, V) differences; x (T, B Sn, W), y (T, B, W)."""
    T, W = x.shape[0], x.shape[-1]
    v, t = x.reshape(T, -1, Sn, W), y
    if path:
        v, t = v.permute(1, 2, 0, 3).reshape(-1, Sn, T * W), y.permute(1, 0, 2).reshape(-1, T * W)
    d2 = (v.unsqueeze(-2) - v.unsqueeze(-3)).square().sum(-1)
    r = torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt() * (d2 > 0)      # (sqrt'(0) = inf: keep the zero pairs out of the graph)
    return (v - t.unsqueeze(-2)).square().sum(-1).sqrt().mean(-1) - r.sum((-2, -1)) / (2 * Sn * (Sn - 1))


say('# tools/time_sample_energy.py: ys (T, B S, W) float32, target (T, B, W); HIP events, variants alternating in one process')
say('# peak = the most allocated during one call above what was allocated when it began; a forward + backward call begins with the previous')
say("# call's gradients (1 x ys + 1 x target) still allocated and frees them first, so its own gradients are not in its figure - for every variant alike")
for T, B, Sn, W, path in ((2, 1024, 8, 128, False), (2, 1024, 32, 128, False), (2, 1024, 128, 128, False), (100, 256, 32, 16, True)):
    gen = torch.Generator().manual_seed(Sn)
    x = torch.randn(T, B * Sn, W, generator=gen).to(dev)
    y = torch.randn(T, B, W, generator=gen).to(dev)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    fwd = {'fused': lambda: S.sample_energy(x, Sn, y, path=path), 'cdist': lambda: engine.sample_energy_tensor_ops(x, Sn, y, path=path)}
    V = T * W if path else W
    if (B if path else T * B) * Sn * Sn * V * 4 < 4 * 2 ** 30:
        fwd['pairwise'] = lambda: pairwise(x, y, Sn, path)

    def train(f):
        def run():
            xg.grad = yg.grad = None
            f(xg, yg).mean().backward()
        return run
    bwd = {'fused': train(lambda a, b: S.sample_energy(a, Sn, b, path=path)),
           'cdist': train(lambda a, b: engine.sample_energy_tensor_ops(a, Sn, b, path=path))}
    if 'pairwise' in fwd:
        bwd['pairwise'] = train(lambda a, b: pairwise(a, b, Sn, path))
    say(f'## (T, B, S, W) = ({T}, {B}, {Sn}, {W}) path={path}: N = {Sn}, V = {V}, {B if path else T * B} scores, ys {x.numel() * 4 / 2 ** 20:.0f} MiB')
    ref = engine.sample_energy_tensor_ops(x.double(), Sn, y.double(), path=path)
    with torch.no_grad():
        for k, f in fwd.items():
            say(f'{k:9s} max |energy - float64 statement| {float((f().double() - ref).abs().max()):.3e}  (energy ~ {float(ref.mean()):.2f})')
        tf = alternate(fwd)
        mf = {k: peak_mb(f) for k, f in fwd.items()}
    tb = alternate(bwd)
    mb = {k: peak_mb(f) for k, f in bwd.items()}
    for k in fwd:
        say(f'forward            {k:9s} {fmt(tf[k])}   peak {mf[k]:9.1f} MiB')
    for k in bwd:
        say(f'forward + backward {k:9s} {fmt(tb[k])}   peak {mb[k]:9.1f} MiB')
    del x, y, xg, yg, ref
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
