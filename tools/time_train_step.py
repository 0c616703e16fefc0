#!/usr/bin/env python3
"""The ordinary K2 training step - (4,17) H = 128, C = 21, 1024 rows, one path per row, 100 Euler steps, in-kernel Philox - as the
whole sdeint + backward() call under HIP events: 200 calls after 20 warm-ups, median / min / p90.  For A/B runs of two checkouts
(the weight-gradient pass, the adjoint): run it from the root of each tree, alternating; it imports the package of the current
directory.

usage (from a repository root): python tools/time_train_step.py"""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import stable_neural_sdes_amd as S
import bench
dev = torch.device('cuda:0')
sde, times, y0 = bench._module(dev, bench.IO, bench.NO, 1024, bench.H, bench.C, bench.L, 3)
ts = torch.tensor([0.0, 100.0], device=dev)
w = torch.randn(2, 1024, bench.H, device=dev)


def step():
    ys = S.sdeint(sde, y0, ts, method='euler', dt=1.0, options={'seed': 7})
    (ys * w).sum().backward()


for _ in range(20):
    step()
torch.cuda.synchronize()
ms = []
for _ in range(5):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(40)]
    for a, b in ev:
        a.record(); step(); b.record()
    torch.cuda.synchronize()
    ms += [a.elapsed_time(b) for a, b in ev]
v = np.array(ms) * 1e3
print(f'{os.path.dirname(os.path.abspath(S.__file__))}: K2 training step, 1024 rows: median {np.median(v):.1f} us  min {v.min():.1f}  p90 {np.percentile(v, 90):.1f}  ({len(v)} calls)')
