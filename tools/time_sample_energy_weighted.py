#!/usr/bin/env python3
"""The energy score of weighted, partially observed sample sets: the weighted and masked variants of the kernel (snsde_sample_energy_weighted /
_backward) against the unweighted kernel at the same shape and against the new tensor-op statement.  Same process, HIP events, the
variants alternating; medians.

At the shapes of profiles/sample_energy_ab.txt - (T, B, S, W) = (2, 1024, S, 128), S in {8, 32, 128}, one score per (time, row), and
path=True at (100, 256, 32, 16), one score per row over the whole path (V = 1600):
  unweighted        engine.sample_energy, no new argument: snsde_sample_energy (the baseline every ratio refers to)
  weighted          log_weight ~ N(0, 4)
  masked            a float mask with about 40 % gaps
  weighted+masked   both
  ops ...           engine.sample_energy_weighted_tensor_ops with the same arguments (where its (.., N, N) planes fit)
forward alone (no_grad) and forward + backward (dL/d ys and dL/d target of the mean score).

usage: python tools/time_sample_energy_weighted.py [output file, default profiles/sample_energy_weighted_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_energy_weighted_ab.txt')
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


def alternate(fns, blocks=8, per=5):
    t = {k: [] for k in fns}
    for f in fns.values():
        event_ms(f, 2)
    for _ in range(blocks):
        for k, f in fns.items():
            t[k] += event_ms(f, per)
    return {k: float(np.median(v)) * 1e3 for k, v in t.items()}


say('# tools/time_sample_energy_weighted.py: ys (T, B S, W) float32, target (T, B, W); HIP events, variants alternating in one process,')
say('# median us of 40 calls; x = the ratio to the unweighted kernel (snsde_sample_energy) of the same row')
for T, B, Sn, W, path in ((2, 1024, 8, 128, False), (2, 1024, 32, 128, False), (2, 1024, 128, 128, False), (100, 256, 32, 16, True)):
    gen = torch.Generator().manual_seed(Sn)
    x = torch.randn(T, B * Sn, W, generator=gen).to(dev)
    y = torch.randn(T, B, W, generator=gen).to(dev)
    lw = (2 * torch.randn(*((B, Sn) if path else (T, B, Sn)), generator=gen)).to(dev)
    mk = (torch.rand(T, B, W, generator=gen) > 0.4).float().to(dev)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    args = {'unweighted': {}, 'weighted': dict(log_weight=lw), 'masked': dict(mask=mk), 'weighted+masked': dict(log_weight=lw, mask=mk)}
    ops_fit = (B if path else T * B) * Sn * Sn * 4 * 4 < 2 * 2 ** 30      # (the weighted statement holds a few (.., N, N) planes)
    call = {k: (lambda a, b, kw=kw: S.sample_energy(a, Sn, b, path=path, **kw)) for k, kw in args.items()}
    if ops_fit:
        for k, kw in list(args.items())[1:]:
            call['ops ' + k] = lambda a, b, kw=kw: engine.sample_energy_weighted_tensor_ops(a, Sn, b, kw.get('log_weight'), kw.get('mask'), path=path)

    def train(f):
        def run():
            xg.grad = yg.grad = None
            f(xg, yg).mean().backward()
        return run
    say(f'## (T, B, S, W) = ({T}, {B}, {Sn}, {W}) path={path}: N = {Sn}, V = {T * W if path else W}, {B if path else T * B} scores')
    ref = engine.sample_energy_weighted_tensor_ops(x.double(), Sn, y.double(), lw.double(), mk.double(), path=path)
    with torch.no_grad():
        got = call['weighted+masked'](x, y)
        say(f'weighted+masked max |energy - float64 statement| {float((got.double() - ref).abs().max()):.3e}  (energy ~ {float(ref.mean()):.2f})')
        tf = alternate({k: (lambda f=f: f(x, y)) for k, f in call.items()})
    tb = alternate({k: train(f) for k, f in call.items()})
    for name, t in (('forward', tf), ('forward + backward', tb)):
        for k in call:
            say(f'{name:18s} {k:20s} median {t[k]:9.1f} us   x {t[k] / t["unweighted"]:6.2f}')
    del x, y, xg, yg, ref, lw, mk
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
