#!/usr/bin/env python3
"""Sample paths (snsde_solve.samples): what the in-place coefficient addressing costs or gains against replicated
coefficients, and snsde_sample_stats against torch's mean / var.  Same process, HIP events, the variants alternating.

  1. the K2 model ((4,17) H = 128, C = 21, 100 Euler steps, in-kernel Philox) at B = 128 input rows x S = 8 paths and
     B = 1024 x S = 4: samples = S with coeffs (B, 100, 84) against samples = 0 with coeffs.repeat_interleave(S) (B S, 100, 84);
     the solve launch alone (prepared workspace reused) and, for the replicated variant, the repeat_interleave itself;
  2. snsde_sample_stats on the (2, B S, H) result against ys.view(2, B, S, H).mean(2) / .var(2).

usage: python tools/time_samples.py [output file, default profiles/time_samples.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_samples.txt')
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
    return f'median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({len(v)} launches)'


say('# tools/time_samples.py: K2 model (io=4, no=17, H=128, C=21, L=101, 100 Euler steps, Philox), HIP events, variants alternating')
for B, Sn in ((128, 8), (1024, 4)):
    pr, _, flat, coeffs, _ = bench.build_inputs(dev, 0, b=B)
    P = B * Sn
    model = engine.model_struct(bench.C, bench.H, bench.H, bench.NL, bench.IO, bench.NO)
    grid = engine.step_grid(np.array([0.0, 100.0], np.float32), 1.0, pr['times'], dev)
    y0 = (0.5 * torch.randn(P, bench.H, generator=torch.Generator().manual_seed(B))).to(dev)
    rep = coeffs.repeat_interleave(Sn, 0).contiguous()
    calls = {'samples=%d, coeffs in place' % Sn: engine.SolveCall(model, flat, coeffs, grid, y0, seed=1, samples=Sn),
             'samples=0, coeffs replicated': engine.SolveCall(model, flat, rep, grid, y0, seed=1)}
    path = engine.forward_path(model, P, bench.L, grid.N, samples=Sn)
    ys = [c.launch().clone() for c in calls.values()]
    torch.cuda.synchronize()
    say(f'## B = {B} input rows x S = {Sn} paths = {P} rows; path {path}; results bit-identical: {bool(torch.equal(ys[0], ys[1]))}')
    ms = {k: [] for k in calls}
    for c in calls.values():
        event_ms(lambda: c.launch(reuse_prepared=True), 10)
    for _ in range(10):      # ten alternating blocks of ten launches
        for k, c in calls.items():
            ms[k] += event_ms(lambda: c.launch(reuse_prepared=True), 10)
    for k, c in calls.items():
        nbytes = c.keep[1].numel() * 4
        say(f'{k:30s} coeffs {nbytes / 1e6:8.2f} MB   solve launch {fmt(ms[k])}')
    event_ms(lambda: coeffs.repeat_interleave(Sn, 0), 5)
    say(f'{"coeffs.repeat_interleave(S)":30s} (what the caller of the replicated variant also pays)   {fmt(event_ms(lambda: coeffs.repeat_interleave(Sn, 0), 50))}')
    a, b = (float(np.median(v)) for v in ms.values())
    say(f'in place / replicated, median solve launch: x{a / b:.3f}; coeffs bytes x{1 / Sn:.3f}')
    # 2. the reduction
    res = ys[0]
    T = res.shape[0]
    m0, v0 = S.sample_stats(res, Sn)
    ref_m, ref_v = res.view(T, B, Sn, bench.H).mean(2), res.view(T, B, Sn, bench.H).var(2)
    torch.cuda.synchronize()
    say(f'snsde_sample_stats on ({T}, {P}, {bench.H}): max |mean - torch| {float((m0 - ref_m).abs().max()):.3e}, '
        f'max |var - torch| / max var {float((v0 - ref_v).abs().max() / ref_v.abs().max()):.3e}')
    t = {'snsde_sample_stats (mean + var)': [], 'torch .mean(2) and .var(2)': []}
    fns = {'snsde_sample_stats (mean + var)': lambda: S.sample_stats(res, Sn),
           'torch .mean(2) and .var(2)': lambda: (res.view(T, B, Sn, bench.H).mean(2), res.view(T, B, Sn, bench.H).var(2))}
    for f in fns.values():
        event_ms(f, 10)
    for _ in range(10):
        for k, f in fns.items():
            t[k] += event_ms(f, 10)
    for k in fns:
        say(f'{k:34s} {fmt(t[k])}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
