#!/usr/bin/env python3
"""What options={'global_rows': N} costs a shard: forward solve of one batch shard planned locally against the same shard planned
for the whole problem (the whole problem's tiles at the shard's occupancy), same process, HIP events, the two alternating.

  K3 shard : (6,17) H = 128, 512 of 4096 rows, 200 Euler steps    - lean 4-row tiles against 16-row tiles (32 workgroups)
  K4 shard : (3,18) H = 64, 1024 of 8192 rows, 71 Euler steps     - wave pairs against 16-row tiles (64 workgroups)
"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import make_problem, param_spec
dev = torch.device('cuda:0')

CFG = [  # name, io, no, NL, shard rows, whole rows, H, C, L
    ('K3 GSDE shard', 6, 17, 2, 512, 4096, 128, 21, 201),
    ('K4 NSDE shard', 3, 18, 2, 1024, 8192, 64, 69, 72),
]


def event_ms(call, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call.launch(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return out


for name, io, no, NL, B, G, H, C, L in CFG:
    pr = make_problem(7, io, no, NL, B, H, C, L, nan_frac=0.2)
    model = engine.model_struct(C, H, H, NL, io, no)
    flat = torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in param_spec(io, no, NL, C, H)])).to(dev)
    grid = engine.step_grid(pr['times'][[0, -1]], 1.0, pr['times'], dev)
    coeffs, y0 = torch.from_numpy(pr['coeffs']).to(dev), torch.from_numpy(pr['y0']).to(dev)
    calls = {g: engine.SolveCall(model, flat, coeffs, grid, y0, seed=1, row_offset=G - B, global_rows=g) for g in (0, G)}
    paths = {g: engine.forward_path(model, B, L, L - 1, global_rows=g, row_offset=G - B) for g in (0, G)}
    for c in calls.values():
        event_ms(c, 5)
    ms = {g: [] for g in calls}
    for _ in range(10):                      # alternate: ten blocks of ten launches each
        for g, c in calls.items():
            ms[g] += event_ms(c, 10)
    for g in (0, G):
        v = np.array(ms[g])
        print(f'{name:14s} B={B:5d} H={H:3d} N={L - 1:3d} global_rows={g:5d} path {paths[g]:7s} forward ms: median {np.median(v):.4f} '
              f'min {v.min():.4f} max {v.max():.4f} (100 launches)')
    print(f'{name:14s} cost of global_rows={G}: x{np.median(ms[G]) / np.median(ms[0]):.2f} (median)')
