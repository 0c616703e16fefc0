#!/usr/bin/env python3
"""Random configurations at H = 256 on 4-row tiles: the two-tile kernels (forward + adjoint + gradients) against the fully streamed
sixteen-wave ones, bit for bit.  A configuration whose plan does not name the two-tile forward AND the two-tile adjoint (no instantiation
for its depth / control blocks: both arms would run the same kernel) is redrawn, so all N cases are real comparisons; the last line says
how many of them ran each two-tile kernel.  usage: python tools/fuzz_h256.py [cases] [seed]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stable_neural_sdes_amd as S
from tests.helpers import make_problem, draw_dW, param_spec
dev = torch.device('cuda:0')
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
ncase = int(sys.argv[1]) if len(sys.argv) > 1 else 40
bad = ci = draws = redrawn = 0
ran = {'lean_two_tile_h256': 0, 'two_tile_h256': 0}
while ci < ncase:
    draws += 1
    assert draws <= 50 * ncase, 'no configuration plans the two-tile kernels'
    io = int(rng.integers(1, 7)); no = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 16, 17]))
    NL = int(rng.integers(1, 4)); C = int(rng.choice([1, 3, 14, 21])); B = int(rng.integers(1, 70)); L = int(rng.integers(3, 12))
    method = str(rng.choice(['euler', 'milstein']))
    pr = make_problem(9000 + draws, io, no, NL, B, 256, C, L, weight_scale=0.7)
    nt = int(rng.integers(2, 5))
    ts = np.sort(rng.choice(np.linspace(0, L - 1, 4 * (L - 1) + 1), size=nt, replace=False)).astype(np.float32)
    dt = float(rng.choice([1.0, 0.5, 0.3]))
    model = S.engine.model_struct(C, 256, 256, NL, io, no)
    flat = torch.from_numpy(np.concatenate([np.asarray(pr['params'][n], np.float32).reshape(-1) for n, _ in param_spec(io, no, NL, C, 256)])).to(dev)
    grid = S.engine.step_grid(ts, dt, pr['times'], dev)
    supplied = torch.from_numpy(draw_dW(9000 + draws, ts, dt, B, 256)).to(dev) if rng.random() < 0.5 else None
    ro = torch.from_numpy(rng.integers(0, nt, size=B).astype(np.int32)).to(dev) if rng.random() < 0.3 else None
    outs = []
    try:
        calls = [S.engine.SolveCall(model, flat, torch.from_numpy(pr['coeffs']).to(dev), grid, torch.from_numpy(pr['y0']).to(dev), dW=supplied,
                                    method=method, seed=11 + draws, kernel='mfma4', stream_all=all_, save_traj=True, save_dW=supplied is None, save_act=True,
                                    row_out=ro) for all_ in (True, False)]
        # (the kernels of the descriptors about to be launched)
        kernels = [(S.engine.forward_kernel(c), S.engine.backward_kernel(c)) for c in calls]
        if kernels[1] != ('lean_two_tile_h256', 'two_tile_h256'):
            redrawn += 1
            continue
        assert kernels[0] == ('lean_streamed_h256', 'general'), kernels
        for call in calls:
            ys = call.launch().clone()
            gy = torch.ones_like(ys) * 0.37 if not outs else outs[0][-1]
            adj, delta = S.engine.solve_backward(call, gy, save_delta=True)
            grad = S.engine.param_gradients(call, adj, delta)
            outs.append((ys, call.traj.clone(), call.act_save.clone(), adj.clone(), delta.clone(), grad.clone(), gy))
    except S._lib.SnsdeError as e:
        print('ERROR', ci, (io, no, NL, C, B, L, method), e)      # (a planned kernel that does not launch is a mismatch, not a redraw)
        bad += 1
        ci += 1
        continue
    ci += 1
    ran['lean_two_tile_h256'] += S.engine.forward_kernel(calls[1]) == 'lean_two_tile_h256'
    ran['two_tile_h256'] += S.engine.backward_kernel(calls[1]) == 'two_tile_h256'
    same = all(torch.equal(x, y) or (torch.isnan(x) == torch.isnan(y)).all() and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) for x, y in zip(outs[0][:6], outs[1][:6]))
    if not same:
        bad += 1
        print('MISMATCH', ci, (io, no, NL, C, B, L, method, ts.tolist(), dt, supplied is not None, ro is not None),
              [bool(torch.equal(x, y)) for x, y in zip(outs[0][:6], outs[1][:6])])
print(f'{ncase} cases, {bad} mismatches')
print(f"two-tile forward {ran['lean_two_tile_h256']} of {ncase}, two-tile adjoint {ran['two_tile_h256']} of {ncase} ({redrawn} configurations redrawn)")
