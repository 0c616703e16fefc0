#!/usr/bin/env python3
"""Sample paths of a model ensemble (SNSDE_FLAG_ENSEMBLE_SAMPLES): M = 8 models of the K2 architecture ((4,17)
H = 128, C = 21, 100 steps of dt = 1, in-kernel Philox, Euler) on 32 input rows x S = 4 paths = 128 paths per member, 1024 paths
in all - ONE sdeint_ensemble(..., options={'samples': 4, 'ensemble_samples': True}) against the only route there was before it,
the M sequential sampled sdeint calls at the same row offsets.  Forward (inference) and training step (forward + backward(),
with 'ensemble_grad' and 'sample_grad').  Same process, HIP events around each arm (host work included), the arms alternating in
ten blocks of ten.  Also the reduction: engine.ensemble_stats of the (T, M, B S, H) result.

usage: python tools/time_ensemble_samples.py [output file, default profiles/time_ensemble_samples.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_ensemble_samples.txt')
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


M, ROWS, SN, method = 8, 32, 4, 'euler'
Bm = ROWS * SN
say(f'# tools/time_ensemble_samples.py: M = {M} models of the K2 architecture (io=4, no=17, H=128, C=21, L=101, 100 steps, Philox, {method}) '
    f'on {ROWS} input rows x S = {SN} paths = {Bm} paths per member, {M * Bm} paths; HIP events around each arm, arms alternating in '
    'ten blocks of ten')
pr, _, _, coeffs, _ = bench.build_inputs(dev, 0, b=ROWS)
times = torch.from_numpy(pr['times']).to(dev)
ts = torch.tensor([0.0, 100.0], device=dev)
sdes = []
for m in range(M):
    torch.manual_seed(10 + m)
    sde = S.Diffusion_model(bench.C, bench.H, bench.H, bench.NL, input_option=bench.IO, noise_option=bench.NO).to(dev)
    sde.set_X(coeffs, times)
    sdes.append(sde)
model = engine.recognise(sdes[0])[0]
L = coeffs.shape[1] + 1
grid = engine.step_grid(np.array([0.0, 100.0], np.float32), 1.0, pr['times'], dev)
y0 = (0.5 * torch.randn(M, Bm, bench.H, generator=torch.Generator().manual_seed(Bm))).to(dev)
cot = torch.randn(2, M, Bm, bench.H, generator=torch.Generator().manual_seed(1)).to(dev)
opts = {'seed': 1, 'samples': SN}
ES = dict(members=M, samples=SN, ensemble_samples=True)

# ---- forward (inference) --------------------------------------------------------------------------------------------------------


def fused_fwd():
    with torch.no_grad():
        return S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0, options=dict(opts, ensemble_samples=True, strict=True))


def sequential_fwd():
    with torch.no_grad():
        return [S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0, options=dict(opts, row_offset=m * Bm, global_rows=M * Bm, strict=True))
                for m in range(M)]


for sde in sdes:
    sde.requires_grad_(False)
same = bool(torch.equal(fused_fwd(), torch.stack(sequential_fwd(), dim=1)))
q = engine.query_descriptor(model, M * Bm, L, grid.N, method, global_rows=M * Bm, **ES)
say(f'## forward; kernel {engine.forward_kernel(q)} ({engine.lean_variant(q)}); results of the two arms bit-identical: {same}')
arms = {'fused: sdeint_ensemble': fused_fwd, f'{M} sequential sampled sdeint': sequential_fwd}
ms = alternate(arms)
for k in arms:
    say(f'{k:42s} {fmt(ms[k])}')
keys = list(arms)
med = {k: float(np.median(v)) for k, v in ms.items()}
say(f'sequential / fused, medians: x{med[keys[1]] / med[keys[0]]:.2f}; fused median below the sequential minimum: {med[keys[0]] < min(ms[keys[1]])}')

ys = fused_fwd()
ms = alternate({'stats': lambda: S.ensemble_stats(ys, M, SN)})
say(f'{"ensemble_stats of the (2, 8, 128, 128) result":42s} {fmt(ms["stats"])}')

# ---- training step --------------------------------------------------------------------------------------------------------------
for sde in sdes:
    sde.requires_grad_(True)
y0.requires_grad_(True)


def zero():
    y0.grad = None
    for sde in sdes:
        for p in sde.parameters():
            p.grad = None


def fused():
    zero()
    out = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0,
                            options=dict(opts, ensemble_samples=True, ensemble_grad=True, sample_grad=True, strict=True))
    (out * cot).sum().backward()


def sequential():
    zero()
    for m in range(M):
        out = S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0,
                       options=dict(opts, sample_grad=True, row_offset=m * Bm, global_rows=M * Bm, strict=True))
        (out * cot[:, m]).sum().backward()


fused()
g_f = [[p.grad.clone() for p in sde.parameters()] for sde in sdes]
y_f = y0.grad.clone()
sequential()
same = bool(torch.equal(y_f, y0.grad)) and all(torch.equal(a, p.grad) for gm, sde in zip(g_f, sdes) for a, p in zip(gm, sde.parameters()))
mode = engine.backward_mode(model, M * Bm, L, grid, method, global_rows=M * Bm, ensemble_grad=True, sample_grad=True, **ES)
q = engine.query_descriptor(model, M * Bm, L, grid.N, method, global_rows=M * Bm, ensemble_grad=True, sample_grad=True, training=True, **ES)
say(f'## training step; backward mode {mode}, kernels {engine.forward_kernel(q)} / {engine.backward_kernel(q)}; gradients of the two arms '
    f'bit-identical: {same}')
arms = {'fused: sdeint_ensemble + backward': fused, f'{M} sequential sampled sdeint + backward': sequential}
ms = alternate(arms)
for k in arms:
    say(f'{k:42s} {fmt(ms[k])}')
keys = list(arms)
med = {k: float(np.median(v)) for k, v in ms.items()}
say(f'sequential / fused, medians: x{med[keys[1]] / med[keys[0]]:.2f}; fused median below the sequential minimum: {med[keys[0]] < min(ms[keys[1]])}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
