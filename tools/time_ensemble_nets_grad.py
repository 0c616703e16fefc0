#!/usr/bin/env python3
"""Training through wave-pair model ensembles (SNSDE_FLAG_ENSEMBLE_NETS_GRAD): M = 8 models of the K4 architecture
((3,18) H = 64, NL = 2, C = 69, L = 72, 71 steps of dt = 1, in-kernel Philox) of 128 rows each on one batch - the whole
sdeint_ensemble(..., options={'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True}) + backward() against the
only route there was before it, 8 sequential sdeint + backward() calls at the same row offsets.  Same process, HIP events around each
arm (host work included: what a training step sees), the arms alternating in ten blocks of ten; Euler and SRK.  For orientation:
ONE model over all 1024 rows.  The tool asserts that the two arms' gradients are bit-identical.

usage: python tools/time_ensemble_nets_grad.py [output file, default profiles/time_ensemble_nets_grad.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_ensemble_nets_grad.txt')
lines = []
IO, NO, H, C_, L, STEPS, M, Bm = 3, 18, 64, 69, 72, 71, 8, 128
THREE = {'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True}


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


say(f'# tools/time_ensemble_nets_grad.py: training step (forward + backward()) of M = {M} models of the K4 architecture (io={IO}, no={NO}, '
    f'H={H}, NL=2, C={C_}, L={L}, {STEPS} steps, Philox) on one batch; HIP events around each arm, arms alternating in ten blocks of ten')
for method in ('euler', 'srk'):
    sde0, times, _ = bench._module(dev, IO, NO, Bm, H, C_, L, 77)
    coeffs = sde0.coeffs
    ts = times[[0, -1]].contiguous()
    sdes = []
    for m in range(M):
        torch.manual_seed(10 + m)
        sde = S.Diffusion_model(C_, H, H, 2, input_option=IO, noise_option=NO).to(dev)
        sde.set_X(coeffs, times)
        sdes.append(sde)
    whole_sde = S.Diffusion_model(C_, H, H, 2, input_option=IO, noise_option=NO).to(dev)
    whole_coeffs = coeffs.repeat(M, 1, 1).contiguous()
    model = engine.recognise(sdes[0])[0]
    grid = engine.step_grid(ts.cpu().numpy(), 1.0, times.cpu().numpy(), dev)
    assert grid.N == STEPS
    y0 = (0.5 * torch.randn(M, Bm, H, generator=torch.Generator().manual_seed(Bm))).to(dev).requires_grad_(True)
    cot = torch.randn(2, M, Bm, H, generator=torch.Generator().manual_seed(1)).to(dev)
    opts = {'seed': 1}

    def zero():
        y0.grad = None
        for sde in sdes + [whole_sde]:
            for p in sde.parameters():
                p.grad = None

    def fused():
        zero()
        ys = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0, options=dict(opts, strict=True, **THREE))
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

    # the two arms compute the same thing: asserted once, bit for bit
    fused()
    g_f = [[p.grad.clone() for p in sde.parameters()] for sde in sdes]
    y_f = y0.grad.clone()
    sequential()
    same = bool(torch.equal(y_f, y0.grad)) and all(torch.equal(a, p.grad) for gm, sde in zip(g_f, sdes) for a, p in zip(gm, sde.parameters()))
    assert same, f'{method}: the gradients of the fused and the sequential arm differ'
    assert float(sdes[0].linear_out.weight.grad.abs().max()) > 0 and float(sdes[0].theta.grad.abs().max()) > 0
    mode = engine.backward_mode(model, M * Bm, L, grid, method, global_rows=M * Bm, members=M, **THREE)
    q = engine.query_descriptor(model, M * Bm, L, grid.N, method, global_rows=M * Bm, members=M, training=True, **THREE)
    say(f'## M = {M} members x {Bm} rows = {M * Bm} rows, {method}; backward mode {mode}, kernels {engine.forward_kernel(q)} / '
        f'{engine.backward_kernel(q)}; gradients of the two arms bit-identical: {same}')
    arms = {
        'fused: sdeint_ensemble + backward': fused,
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
