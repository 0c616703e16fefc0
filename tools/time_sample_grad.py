#!/usr/bin/env python3
"""Training through sample paths (options={'samples': S, 'sample_grad': True}): the whole sdeint + backward() call at
the K2 model ((4,17) H = 128, C = 21, 100 Euler steps, in-kernel Philox) with the coefficients in place against the replicated
route - the caller's repeat_interleave of the coefficients in front of the ordinary differentiable solve, which is what the
parent commit offers - at 128 input rows x 8 paths and 1024 x 4, with and without coeffs.requires_grad.  Same process, HIP events
around the whole call, 100 calls per variant in ten alternating blocks of ten; peak allocated bytes of one call of each route; and
the coefficient-gradient entry point alone against "replicated kernel + sum over S".

usage: python tools/time_sample_grad.py [output file, default profiles/time_sample_grad.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_sample_grad.txt')
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
    return f'median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({len(v)} calls)'


say('# tools/time_sample_grad.py: K2 model (io=4, no=17, H=128, C=21, L=101, 100 Euler steps, Philox), whole sdeint + backward() call,')
say('# HIP events, ten alternating blocks of ten calls per variant')
ts = torch.tensor([0.0, 100.0], device=dev)
for B, Sn in ((128, 8), (1024, 4)):
    P = B * Sn
    sde, times, _ = bench._module(dev, bench.IO, bench.NO, B, bench.H, bench.C, bench.L, 3)
    model = engine.recognise(sde)[0]
    grid = engine.step_grid(np.array([0.0, 100.0], np.float32), 1.0, S.torchsde._HostTimes.get(times), dev)
    mode = engine.backward_mode(model, P, bench.L, grid, 'euler', samples=Sn, sample_grad=True)
    base = sde.coeffs.detach()
    y0 = (0.5 * torch.randn(P, bench.H, generator=torch.Generator().manual_seed(B))).to(dev)
    w = torch.randn(2, P, bench.H, generator=torch.Generator().manual_seed(B + 1)).to(dev)
    say(f'## B = {B} input rows x S = {Sn} paths = {P} rows; sampled backward mode {mode}; coeffs in place {base.numel() * 4 / 1e6:.2f} MB, '
        f'replicated {base.numel() * 4 * Sn / 1e6:.2f} MB (x{Sn}: the gradient likewise)')
    for cgrad in (False, True):
        coeffs = base.clone().requires_grad_(cgrad)

        def in_place():
            sde.set_X(coeffs, times)
            ys = S.sdeint(sde, y0, ts, method='euler', dt=1.0, options={'samples': Sn, 'sample_grad': True, 'seed': 7})
            (ys * w).sum().backward()
            return ys

        def replicated():
            sde.set_X(coeffs.repeat_interleave(Sn, 0), times)
            ys = S.sdeint(sde, y0, ts, method='euler', dt=1.0, options={'seed': 7})
            (ys * w).sum().backward()
            return ys
        fns = {'coeffs in place (samples, sample_grad)': in_place, 'coeffs replicated (repeat_interleave)': replicated}
        res, peak = {}, {}
        for k, f in fns.items():
            for p in sde.parameters():
                p.grad = None
            coeffs.grad = None
            f()      # (warm: caches, allocator)
            for p in sde.parameters():
                p.grad = None
            coeffs.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            ys = f()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated(dev) - before
            res[k] = (ys.detach().clone(), [p.grad.clone() for p in sde.parameters()], None if coeffs.grad is None else coeffs.grad.clone())
            del ys
        a, b = res.values()
        same = torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
        cerr = ''
        if cgrad:
            cerr = f'; coeffs.grad max |in place - replicated| / max {float((a[2] - b[2]).abs().max() / b[2].abs().max()):.2e}'
        say(f'### coeffs.requires_grad = {cgrad}: states and parameter gradients bit-identical: {same}{cerr}')
        ms = {k: [] for k in fns}
        for _ in range(10):
            for k, f in fns.items():
                ms[k] += event_ms(f, 10)
        for k in fns:
            say(f'{k:40s} {fmt(ms[k])}   peak allocated {peak[k] / 1e6:8.1f} MB')
        ma, mb = (float(np.median(v)) for v in ms.values())
        pa, pb = peak.values()
        say(f'in place / replicated: median call x{ma / mb:.3f}, peak allocated x{pa / pb:.3f}')
    # the coefficient-gradient entry point alone, on the planes of one adjoint: in place against replicated kernel + sum over S
    flat = engine.flatten_params(sde, *engine.recognise(sde)[1:], dev)
    kw = dict(seed=7, save_traj=True, save_act=True)
    ca = engine.SolveCall(model, flat, base, grid, y0, samples=Sn, sample_grad=True, **kw)
    cb = engine.SolveCall(model, flat, base.repeat_interleave(Sn, 0).contiguous(), grid, y0, **kw)
    outs = []
    for c in (ca, cb):
        c.launch()
        adj, _, delta = engine.backward_with_gradients(c, w, return_delta=True)
        outs.append((c, adj, delta))
    fa = lambda: engine.coeff_gradients(*outs[0])
    fb = lambda: engine.coeff_gradients(*outs[1]).view(B, Sn, *base.shape[1:]).sum(1)
    ga, gb = fa(), fb()
    torch.cuda.synchronize()
    say(f'### snsde_coeff_gradients alone (same delta planes: {bool(torch.equal(outs[0][2], outs[1][2]))}); '
        f'max |in place - (replicated, summed)| / max {float((ga - gb).abs().max() / gb.abs().max()):.2e}')
    t = {'in place (B rows out)': [], 'replicated kernel + sum over S': []}
    for f in (fa, fb):
        event_ms(f, 5)
    for _ in range(10):
        t['in place (B rows out)'] += event_ms(fa, 10)
        t['replicated kernel + sum over S'] += event_ms(fb, 10)
    for k, v in t.items():
        say(f'{k:40s} {fmt(v)}')
    del outs, ca, cb
open(out_path, 'w').write('\n'.join(lines) + '\n')
