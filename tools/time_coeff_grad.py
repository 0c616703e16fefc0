#!/usr/bin/env python3
"""What dL/d coeffs costs on the K2 training step (snsde_coeff_gradients): the bench's K2 training leg ((4,17)
H = 128, C = 21, 1024 rows, 100 Euler steps, Philox increments, forward + fused adjoint + native weight gradients) with and
without `coeffs.requires_grad`.  Same process, HIP events, the two variants alternating in blocks of ten steps; then the
snsde_coeff_gradients call alone on the planes of one finished backward.

usage: python tools/time_coeff_grad.py [output file, default profiles/time_coeff_grad.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_coeff_grad.txt')
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
    return f'median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({len(v)} steps)'


sde, times, y0 = bench._module(dev, bench.IO, bench.NO, bench.B, bench.H, bench.C, bench.L, 77)
ts = times[[0, -1]]
params = list(sde.parameters())
opts = {'seed': 5, 'strict': True}
base = sde.coeffs.detach()
leaf = base.clone().requires_grad_(True)


def step(coeffs):
    sde.set_X(coeffs, times)
    for p in params:
        p.grad = None
    leaf.grad = None
    yy = y0.clone().requires_grad_(True)
    S.torchsde.sdeint(sde, yy, ts, dt=1.0, method='euler', options=opts)[-1].square().mean().backward()


variants = {'coeffs.requires_grad = False (the step of the parent commit)': lambda: step(base),
            'coeffs.requires_grad = True  (+ snsde_coeff_gradients)': lambda: step(leaf)}
say(f'# tools/time_coeff_grad.py: K2 training step (io={bench.IO}, no={bench.NO}, H={bench.H}, C={bench.C}, {bench.B} rows, '
    f'{bench.L - 1} Euler steps, Philox), whole sdeint forward + backward call, HIP events, variants alternating')
ms = {k: [] for k in variants}
for f in variants.values():
    event_ms(f, 10)
assert leaf.grad is not None and float(leaf.grad.abs().max()) > 0
for _ in range(10):
    for k, f in variants.items():
        ms[k] += event_ms(f, 10)
for k in variants:
    say(f'{k:66s} {fmt(ms[k])}')
a, b = (float(np.median(v)) for v in ms.values())
say(f'cost of the coefficient gradient on the whole step: {1e3 * (b - a):+.1f} us (x{b / a:.3f})')

# the entry point alone, on the delta planes of one finished backward
model, layout, numel = engine.recognise(sde)
flat = engine.flatten_params(sde, layout, numel, dev)
grid = engine.step_grid(ts.cpu().numpy(), 1.0, S.torchsde._HostTimes.get(times), dev)
call = engine.SolveCall(model, flat, base.contiguous(), grid, y0, seed=5, save_traj=True, save_dW=True, save_act=True)
ys = call.launch()
adj, _, delta = engine.backward_with_gradients(call, torch.ones_like(ys), return_delta=True)
event_ms(lambda: engine.coeff_gradients(call, adj, delta), 10)
t = event_ms(lambda: engine.coeff_gradients(call, adj, delta), 100)
nbytes = delta[:, 0].numel() * 4
say(f'snsde_coeff_gradients alone (memset + fold + vjp + walk; reads one delta plane per pass = {nbytes / 1e6:.1f} MB): {fmt(t)}')
say(f'  = {nbytes / (np.median(t) * 1e-3) / 1e9:.0f} GB/s on that read')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
