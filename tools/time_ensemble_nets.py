#!/usr/bin/env python3
"""Model ensembles on the wave-pair and diffusion-net kernels (SNSDE_FLAG_ENSEMBLE_NETS): M = 8 models of the K4
architecture ((3,18) H = 64, NL = 2, C = 69, L = 72, 71 steps of dt = 1, in-kernel Philox) on one batch - the fused solve (option
on) against the loop of 8 solves at the same row offsets (option off: the only route there was before it).  Same process, HIP
events around the solve calls alone (SolveCall.launch: the descriptors are built once), 100 calls per arm in alternating blocks
of ten.

  wave pairs (H = 64): 8 models x 128 rows, and 8 x 32 input rows x 4 sample paths, under Euler and SRK;
  snsde_m4n_kernel:    SRK at H = 128, 8 models x 128 rows.

usage: python tools/time_ensemble_nets.py [output file, default profiles/time_ensemble_nets.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_ensemble_nets.txt')
lines = []
IO, NO, C_, L, STEPS, M = 3, 18, 69, 72, 71, 8


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


say(f'# tools/time_ensemble_nets.py: M = {M} models of the K4 architecture (io={IO}, no={NO}, NL=2, C={C_}, L={L}, {STEPS} steps, Philox) on one '
    'batch; HIP events around the solve calls alone, 100 calls per arm in alternating blocks of ten')
for H, B, Sn, method in ((64, 128, 1, 'euler'), (64, 128, 1, 'srk'), (64, 32, 4, 'euler'), (64, 32, 4, 'srk'), (128, 128, 1, 'srk')):
    Bm = B * Sn
    sde0, times, _ = bench._module(dev, IO, NO, B, H, C_, L, 77)
    coeffs = sde0.coeffs
    sdes = []
    for m in range(M):
        torch.manual_seed(10 + m)
        sde = S.Diffusion_model(C_, H, H, 2, input_option=IO, noise_option=NO).to(dev).requires_grad_(False)
        sde.set_X(coeffs, times)
        sdes.append(sde)
    model = engine.recognise(sdes[0])[0]
    flats = [engine.flatten_params(sde, *engine.recognise(sde)[1:], dev) for sde in sdes]
    ends = times[[0, -1]].cpu().numpy()
    grid = engine.step_grid(ends, 1.0, times.cpu().numpy(), dev)
    assert grid.N == STEPS
    y0 = (0.5 * torch.randn(M, Bm, H, generator=torch.Generator().manual_seed(Bm))).to(dev)
    rows = y0.reshape(M * Bm, H).contiguous()
    fused = engine.SolveCall(model, torch.stack(flats), coeffs, grid, rows, method=method, seed=1, members=M, ensemble_nets=True,
                             samples=Sn if Sn > 1 else 0, ensemble_samples=Sn > 1)
    # the loop: member m alone as a shard of the whole (sample paths: on the coefficients replicated path-major, as sdeint does where
    # the kernel does not map paths to input rows)
    cm = coeffs.repeat_interleave(Sn, dim=0).contiguous() if Sn > 1 else coeffs
    parts = [engine.SolveCall(model, flats[m], cm, grid, y0[m].contiguous(), method=method, seed=1, row_offset=m * Bm, global_rows=M * Bm)
             for m in range(M)]
    whole = engine.SolveCall(model, flats[0], cm.repeat(M, 1, 1).contiguous(), grid, rows, method=method, seed=1)
    a = fused.launch().clone()
    b = torch.cat([p.launch() for p in parts], dim=1)
    torch.cuda.synchronize()
    say(f'## H = {H}: {M} members x {B} rows' + (f' x {Sn} paths' if Sn > 1 else '') + f' = {M * Bm} rows, {method}; kernel '
        f'{engine.forward_kernel(fused)} (members alone: {engine.forward_kernel(parts[0])}, one model on all rows: '
        f'{engine.forward_kernel(whole)}); results bit-identical: {bool(torch.equal(a, b))}')
    arms = {
        f'fused, SolveCall(members={M})': lambda: fused.launch(),
        f'loop of {M} SolveCalls': lambda: [p.launch() for p in parts],
        f'one model, {M * Bm} rows': lambda: whole.launch(),
        f'one model, {Bm} rows (one of the {M})': lambda: parts[0].launch(),
    }
    with torch.no_grad():
        ms = alternate(arms)
    for k in arms:
        say(f'{k:36s} {fmt(ms[k])}')
    med = {k: float(np.median(v)) for k, v in ms.items()}
    keys = list(arms)
    say(f'loop / fused, medians: x{med[keys[1]] / med[keys[0]]:.2f}; fused / one model on {M * Bm} rows x{med[keys[0]] / med[keys[2]]:.2f}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
