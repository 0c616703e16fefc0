#!/usr/bin/env python3
"""What differentiating through the spline coefficient construction costs ("dL/dX"): the HIP adjoint
(snsde_natural_cubic_coeffs_backward / snsde_hermite_coeffs_backward behind one autograd node) against autograd through the
tensor-op construction (SNSDE_SPLINE_GRAD=torch, the route of the parent commit).

  1. X -> coeffs -> (coeffs * w).sum().backward() at K2 (1024 x 101 x 21) and at a small shape (64 x 17 x 5), both kinds,
     without missing values and with 20 % of them;
  2. the K2 training step through sdeint ((4,17) H = 128, 100 Euler steps, Philox) with X.requires_grad, natural coefficients.

Same process, HIP events around the whole step (host time of the tensor-op route's many small launches and of its host
synchronisations is inside the interval), the two routes alternating in blocks.

usage: python tools/time_spline_grad.py [output file, default profiles/time_spline_grad.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_spline_grad.txt')
lines = []
ROUTES = ('native', 'torch')


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
    return f'median {np.median(v):10.1f} us  min {v.min():10.1f}  max {v.max():10.1f}  ({len(v)} steps)'


def with_route(route, fn):
    def run():
        os.environ['SNSDE_SPLINE_GRAD'] = route
        try:
            fn()
        finally:
            os.environ.pop('SNSDE_SPLINE_GRAD', None)
    return run


def alternate(fn, blocks, per_block, warm=2):
    runs = {r: with_route(r, fn) for r in ROUTES}
    for f in runs.values():
        event_ms(f, warm)
    ms = {r: [] for r in ROUTES}
    for _ in range(blocks):
        for r, f in runs.items():
            ms[r] += event_ms(f, per_block)
    return ms


def coeffs_of(kind, t, X):
    if kind == 'natural':
        return torch.cat(S.controldiffeq.natural_cubic_spline_coeffs(t, X), dim=-1)
    return S.torchcde.hermite_cubic_coefficients_with_backward_differences(X, t)


def data(B, L, Cn, nan_frac, seed=3):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((B, L, Cn)) * 0.1).cumsum(1).astype(np.float32)
    if nan_frac > 0:
        X[rng.random((B, L, Cn)) < nan_frac] = np.nan
    return (torch.arange(L, dtype=torch.float32, device=dev), torch.from_numpy(X).to(dev).requires_grad_(True),
            torch.from_numpy(rng.standard_normal((B, L - 1, 4 * Cn)).astype(np.float32)).to(dev))


say('# tools/time_spline_grad.py: X -> coeffs -> (coeffs * w).sum().backward(), forward + backward of the construction, HIP events,')
say('# native = HIP construction + HIP adjoint in one autograd node; torch = autograd through the tensor-op construction')
for nan_frac in (0.0, 0.2):
    for name, (B, L, Cn) in (('K2', (bench.B, bench.L, bench.C)), ('small', (64, 17, 5))):
        for kind in ('natural', 'hermite'):
            t, X, w = data(B, L, Cn, nan_frac)
            grads = {}

            def step():
                X.grad = None
                (coeffs_of(kind, t, X) * w).sum().backward()
                grads[os.environ['SNSDE_SPLINE_GRAD']] = X.grad

            ms = alternate(step, blocks=5, per_block=4)
            err = float((grads['native'] - grads['torch']).abs().max()) / float(grads['torch'].abs().max())
            for r in ROUTES:
                say(f'{name:5s} {B:4d} x {L:3d} x {Cn:2d} {kind:8s} missing {int(100 * nan_frac):2d} % {r:7s} {fmt(ms[r])}')
            a, b = (float(np.median(ms[r])) for r in ROUTES)
            say(f'{name:5s} {kind:8s} missing {int(100 * nan_frac):2d} %: native / torch = x{a / b:.4f} (torch / native = x{b / a:.1f}); '
                f'max |native - torch| / max |torch| = {err:.2e}')

# ---- the two adjoint entry points alone
say('# engine.spline_coeffs_backward alone at K2, 20 % missing (one launch; bytes = grad_coeffs and X read, grad_X written)')
for kind in ('natural', 'hermite'):
    t, X, w = data(bench.B, bench.L, bench.C, 0.2)
    Xd = X.detach()
    event_ms(lambda: S.engine.spline_coeffs_backward(t, Xd, w, kind), 10)
    v = event_ms(lambda: S.engine.spline_coeffs_backward(t, Xd, w, kind), 100)
    nbytes = 4 * (w.numel() + 2 * Xd.numel())
    say(f'K2    {kind:8s} adjoint call {fmt(v)}  {nbytes / 1e6:.1f} MB = {nbytes / (np.median(v) * 1e-3) / 1e9:.0f} GB/s')

# ---- the K2 training step with X.requires_grad
sde, times, y0 = bench._module(dev, bench.IO, bench.NO, bench.B, bench.H, bench.C, bench.L, 77)
ts = times[[0, -1]]
params = list(sde.parameters())
opts = {'seed': 5, 'strict': True}
_, X, _ = data(bench.B, bench.L, bench.C, 0.2, seed=77)
base = sde.coeffs.detach()


def train_step(differentiate=True):
    X.grad = None
    for p in params:
        p.grad = None
    coeffs = coeffs_of('natural', times, X) if differentiate else base
    sde.set_X(coeffs, times)
    yy = y0.clone().requires_grad_(True)
    S.torchsde.sdeint(sde, yy, ts, dt=1.0, method='euler', options=opts)[-1].square().mean().backward()


say(f'# K2 training step (io={bench.IO}, no={bench.NO}, H={bench.H}, C={bench.C}, {bench.B} rows, {bench.L - 1} Euler steps, Philox): '
    f'natural coefficients from X (20 % missing) + sdeint forward + backward down to X.grad')
ms = alternate(train_step, blocks=5, per_block=4)
assert X.grad is not None and float(X.grad.abs().max()) > 0
fixed = event_ms(lambda: train_step(False), 5) and event_ms(lambda: train_step(False), 20)
say(f'coefficients fixed (no construction in the step, coeffs.requires_grad = False)   {fmt(fixed)}')
for r in ROUTES:
    say(f'X.requires_grad, SNSDE_SPLINE_GRAD={r:7s}                                        {fmt(ms[r])}')
a, b = (float(np.median(ms[r])) for r in ROUTES)
say(f'training step through X: native / torch = x{a / b:.4f} (torch / native = x{b / a:.1f})')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
