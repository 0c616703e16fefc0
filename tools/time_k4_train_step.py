#!/usr/bin/env python3
"""The ordinary K4 training step - (3,18) H = 64, NL = 2, C = 69, 2048 rows, 71 steps of dt = 1, in-kernel Philox, the wave-pair
kernels - as the whole sdeint + backward() call under HIP events, Euler and SRK: 200 calls after 20 warm-ups, median / min / p90
and the medians of the five blocks of 40 calls.
For A/B runs of two checkouts (tools/time_train_step.py is the K2 form): run it from the root of each tree, alternating; it imports
the package of the current directory.

usage (from a repository root): python <path to>/time_k4_train_step.py"""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import stable_neural_sdes_amd as S
import bench
dev = torch.device('cuda:0')
sde, times, y0 = bench._module(dev, 3, 18, 2048, 64, 69, 72, 77)
ts = times[[0, -1]].contiguous()
w = torch.randn(2, 2048, 64, device=dev)
for method in ('euler', 'srk'):
    def step():
        ys = S.sdeint(sde, y0, ts, method=method, dt=1.0, options={'seed': 7, 'strict': True})
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
    blocks = ' '.join(f'{np.median(v[i:i + 40]):.0f}' for i in range(0, len(v), 40))
    print(f'K4 train step {method:5s} 2048 rows: median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({len(v)} runs; medians of the five blocks of 40: {blocks})', flush=True)
