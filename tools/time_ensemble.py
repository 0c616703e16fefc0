#!/usr/bin/env python3
"""Model ensembles (snsde_solve.members): M models of the K2 architecture ((4,17) H = 128, C = 21, 100 steps of
dt = 1, in-kernel Philox) on one batch - the fused ensemble solve against the only route there was before it, M sequential solves
at the same row offsets.  Same process, HIP events around each arm, the arms alternating in blocks.

  M = 8 x 128 rows and M = 4 x 256 rows under Euler, M = 8 x 128 under SRK.  Per configuration:
  1. engine level, prepare launch included (every one of the M sequential sdeint calls pays its own): one SolveCall(members=M)
     launch against M SolveCall launches; the same with the prepared workspaces reused (what the prepare launches cost); and ONE
     model on all M Bm rows, the solve the stacked call is expected to approach;
  2. front end: sdeint_ensemble against the loop of M sdeint calls (host work included: what a caller sees).

usage: python tools/time_ensemble.py [output file, default profiles/time_ensemble.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_ensemble.txt')
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
    return f'median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({len(v)} runs)'


def alternate(arms, blocks=10, per_block=10):
    ms = {k: [] for k in arms}
    for f in arms.values():
        event_ms(f, 5)
    for _ in range(blocks):
        for k, f in arms.items():
            ms[k] += event_ms(f, per_block)
    return ms


say('# tools/time_ensemble.py: M models of the K2 architecture (io=4, no=17, H=128, C=21, L=101, 100 steps, Philox) on one batch; HIP events '
    'around each arm, arms alternating in ten blocks of ten')
for M, Bm, method in ((8, 128, 'euler'), (4, 256, 'euler'), (8, 128, 'srk')):
    pr, _, _, coeffs, _ = bench.build_inputs(dev, 0, b=Bm)
    times = torch.from_numpy(pr['times']).to(dev)
    ts = torch.tensor([0.0, 100.0], device=dev)
    sdes = []
    for m in range(M):
        torch.manual_seed(10 + m)
        sde = S.Diffusion_model(bench.C, bench.H, bench.H, bench.NL, input_option=bench.IO, noise_option=bench.NO).to(dev).requires_grad_(False)
        sde.set_X(coeffs, times)
        sdes.append(sde)
    model = engine.recognise(sdes[0])[0]
    flats = [engine.flatten_params(sde, *engine.recognise(sde)[1:], dev) for sde in sdes]
    stacked = torch.stack(flats)
    grid = engine.step_grid(np.array([0.0, 100.0], np.float32), 1.0, pr['times'], dev)
    y0 = (0.5 * torch.randn(M, Bm, bench.H, generator=torch.Generator().manual_seed(Bm))).to(dev)
    rows = y0.reshape(M * Bm, bench.H).contiguous()
    fused = engine.SolveCall(model, stacked, coeffs, grid, rows, method=method, seed=1, members=M)
    parts = [engine.SolveCall(model, flats[m], coeffs, grid, y0[m].contiguous(), method=method, seed=1, row_offset=m * Bm,
                              global_rows=M * Bm) for m in range(M)]
    whole = engine.SolveCall(model, flats[0], coeffs.repeat(M, 1, 1).contiguous(), grid, rows, method=method, seed=1)
    a = fused.launch().clone()
    b = torch.cat([p.launch() for p in parts], dim=1)
    torch.cuda.synchronize()
    say(f'## M = {M} members x {Bm} rows = {M * Bm} rows, {method}; kernel {engine.forward_kernel(fused)} (members: {engine.forward_kernel(parts[0])}, '
        f'one model on all rows: {engine.forward_kernel(whole)}); results bit-identical: {bool(torch.equal(a, b))}')
    opts = {'seed': 1}
    arms = {
        f'fused, SolveCall(members={M})': lambda: fused.launch(),
        f'{M} sequential SolveCalls': lambda: [p.launch() for p in parts],
        f'fused, prepared blocks reused': lambda: fused.launch(reuse_prepared=True),
        f'{M} sequential, prepared reused': lambda: [p.launch(reuse_prepared=True) for p in parts],
        f'one model, {M * Bm} rows': lambda: whole.launch(),
        f'one model, {Bm} rows (one of the {M})': lambda: parts[0].launch(),
        'front end: sdeint_ensemble': lambda: S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0, options=opts),
        f'front end: {M} sdeint calls': lambda: [S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0,
                                                          options=dict(opts, row_offset=m * Bm, global_rows=M * Bm)) for m in range(M)],
    }
    with torch.no_grad():
        ms = alternate(arms)
    for k in arms:
        say(f'{k:36s} {fmt(ms[k])}')
    med = {k: float(np.median(v)) for k, v in ms.items()}
    keys = list(arms)
    say(f'sequential / fused, medians: engine x{med[keys[1]] / med[keys[0]]:.2f} (prepared reused x{med[keys[3]] / med[keys[2]]:.2f}), '
        f'front end x{med[keys[7]] / med[keys[6]]:.2f}; fused / one model on {M * Bm} rows x{med[keys[0]] / med[keys[4]]:.2f}; '
        f'prepare launch: fused {1e3 * (med[keys[0]] - med[keys[2]]):.1f} us, sequential {1e3 * (med[keys[1]] - med[keys[3]]):.1f} us')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
