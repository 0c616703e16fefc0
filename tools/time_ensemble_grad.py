#!/usr/bin/env python3
"""Training through model ensembles (SNSDE_FLAG_ENSEMBLE_GRAD): M models of the K2 architecture ((4,17) H = 128,
C = 21, 100 steps of dt = 1, in-kernel Philox) on one batch - the whole sdeint_ensemble(..., options={'ensemble_grad': True}) +
backward() against the only route there was before it, M sequential sdeint + backward() calls at the same row offsets.  Same
process, HIP events around each arm (host work included: what a training step sees), the arms alternating in ten blocks of ten.

  M = 8 x 128 rows and M = 4 x 256 rows under Euler, M = 8 x 128 under SRK.  For orientation: ONE model over all M Bm rows.

usage: python tools/time_ensemble_grad.py [output file, default profiles/time_ensemble_grad.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_ensemble_grad.txt')
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
    return f'median {np.median(v):8.1f} us  min {v.min():8.1f}  max {v.max():8.1f}  ({len(v)} runs)'


def alternate(arms, blocks=10, per_block=10):
    ms = {k: [] for k in arms}
    for f in arms.values():
        event_ms(f, 5)
    for _ in range(blocks):
        for k, f in arms.items():
            ms[k] += event_ms(f, per_block)
    return ms


say('# tools/time_ensemble_grad.py: training step (forward + backward()) of M models of the K2 architecture (io=4, no=17, H=128, C=21, L=101, '
    '100 steps, Philox) on one batch; HIP events around each arm, arms alternating in ten blocks of ten')
for M, Bm, method in ((8, 128, 'euler'), (4, 256, 'euler'), (8, 128, 'srk')):
    pr, _, _, coeffs, _ = bench.build_inputs(dev, 0, b=Bm)
    times = torch.from_numpy(pr['times']).to(dev)
    ts = torch.tensor([0.0, 100.0], device=dev)
    sdes = []
    for m in range(M):
        torch.manual_seed(10 + m)
        sde = S.Diffusion_model(bench.C, bench.H, bench.H, bench.NL, input_option=bench.IO, noise_option=bench.NO).to(dev)
        sde.set_X(coeffs, times)
        sdes.append(sde)
    whole_sde = S.Diffusion_model(bench.C, bench.H, bench.H, bench.NL, input_option=bench.IO, noise_option=bench.NO).to(dev)
    whole_coeffs = coeffs.repeat(M, 1, 1).contiguous()
    model = engine.recognise(sdes[0])[0]
    grid = engine.step_grid(np.array([0.0, 100.0], np.float32), 1.0, pr['times'], dev)
    y0 = (0.5 * torch.randn(M, Bm, bench.H, generator=torch.Generator().manual_seed(Bm))).to(dev).requires_grad_(True)
    cot = torch.randn(2, M, Bm, bench.H, generator=torch.Generator().manual_seed(1)).to(dev)
    opts = {'seed': 1}

    def zero():
        y0.grad = None
        for sde in sdes + [whole_sde]:
            for p in sde.parameters():
                p.grad = None

    def fused():
        zero()
        ys = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0, options=dict(opts, ensemble_grad=True, strict=True))
        (ys * cot).sum().backward()

    def sequential():
        zero()
        for m in range(M):
            ys = S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0, options=dict(opts, row_offset=m * Bm, global_rows=M * Bm, strict=True))
            (ys * cot[:, m]).sum().backward()

    def one_model():
        zero()
        whole_sde.set_X(whole_coeffs, times)
        ys = S.sdeint(whole_sde, y0.reshape(M * Bm, -1), ts, method=method, dt=1.0, options=dict(opts, strict=True))
        (ys * cot.reshape(2, M * Bm, -1)).sum().backward()

    # the two arms compute the same thing: checked once, bit for bit
    fused()
    g_f = [[p.grad.clone() for p in sde.parameters()] for sde in sdes]
    y_f = y0.grad.clone()
    sequential()
    same = bool(torch.equal(y_f, y0.grad)) and all(torch.equal(a, p.grad) for gm, sde in zip(g_f, sdes) for a, p in zip(gm, sde.parameters()))
    mode = engine.backward_mode(model, M * Bm, coeffs.shape[1] + 1, grid, method, global_rows=M * Bm, members=M, ensemble_grad=True)
    q = engine.query_descriptor(model, M * Bm, coeffs.shape[1] + 1, grid.N, method, global_rows=M * Bm, members=M, ensemble_grad=True, training=True)
    say(f'## M = {M} members x {Bm} rows = {M * Bm} rows, {method}; backward mode {mode}, kernels {engine.forward_kernel(q)} / '
        f'{engine.backward_kernel(q)}; gradients of the two arms bit-identical: {same}')
    arms = {
        f'fused: sdeint_ensemble + backward': fused,
        f'{M} sequential sdeint + backward': sequential,
        f'one model, {M * Bm} rows, + backward': one_model,
    }
    ms = alternate(arms)
    for k in arms:
        say(f'{k:38s} {fmt(ms[k])}')
    keys = list(arms)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ok = med[keys[0]] < min(ms[keys[1]])
    say(f'sequential / fused, medians: x{med[keys[1]] / med[keys[0]]:.2f}; fused / one model on {M * Bm} rows x{med[keys[0]] / med[keys[2]]:.2f}; '
        f'fused median below the sequential minimum: {ok}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
