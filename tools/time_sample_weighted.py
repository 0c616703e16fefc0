#!/usr/bin/env python3
"""Weighted sample sets: sample_stats / sample_crps / sample_quantiles with log_weight= (the kernels of
csrc/snsde_weighted.hip) against their unweighted siblings and against the same definitions in tensor ops
(engine.sample_*_weighted_tensor_ops).  Same process, HIP events, the variants alternating.

Shapes (T, B, W) = (2, 1024, 128), S = 8 | 32 | 128 paths per row: ys (T, B S, W), log_weight (T, B, S) ~ N(0, 1), target (T, B, W),
the five levels (0, 0.1, 0.5, 0.9, 1).  Forward, and forward + backward (an upstream gradient of ones through autograd).
  weighted    the function with log_weight= on CUDA float32 (one launch forward, one backward)
  unweighted  the same function without weights (the existing kernels)
  ops         the weighted definition in tensor ops (softmax-style weights, sort, cumsum, gather, where)
There is no gate: the file says what was measured.

usage: python tools/time_sample_weighted.py [output file, default profiles/sample_weighted_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S  # noqa: F401
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_weighted_ab.txt')
LEVELS = (0.0, 0.1, 0.5, 0.9, 1.0)
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
    return f'median {np.median(v):9.1f} us  min {v.min():9.1f}  p90 {np.percentile(v, 90):9.1f}  ({len(v)} calls)'


def alternate(fns, blocks=6, per=5):
    t = {k: [] for k in fns}
    for f in fns.values():
        event_ms(f, 3)
    for _ in range(blocks):
        for k, f in fns.items():
            t[k] += event_ms(f, per)
    return t


def total(out):
    outs = out if isinstance(out, (tuple, list)) else (out,)
    return sum(o.sum() for o in outs if o is not None)


say('# tools/time_sample_weighted.py: ys (T, B S, W) float32, log_weight (T, B, S), target (T, B, W) on the device; HIP events, the variants')
say('# alternating in one process (six blocks of five calls each); fwd = the call under no_grad, fwd+bwd = the call and autograd.grad')
T, B, W = 2, 1024, 128
for Sn in (8, 32, 128):
    gen = torch.Generator().manual_seed(Sn)
    x = torch.randn(T, B * Sn, W, generator=gen).to(dev)
    lw, y = torch.randn(T, B, Sn, generator=gen).to(dev), torch.randn(T, B, W, generator=gen).to(dev)
    xg = x.clone().requires_grad_(True)
    say(f'## (T, B, W) = ({T}, {B}, {W}), S = {Sn}: ys {x.numel() * 4 / 2 ** 20:.1f} MiB')
    calls = {
        'stats': {'weighted': lambda v: engine.sample_stats(v, Sn, log_weight=lw), 'unweighted': lambda v: engine.sample_stats(v, Sn),
                  'ops': lambda v: engine.sample_stats_weighted_tensor_ops(v, Sn, lw)},
        'crps': {'weighted': lambda v: engine.sample_crps(v, Sn, y, log_weight=lw), 'unweighted': lambda v: engine.sample_crps(v, Sn, y),
                 'ops': lambda v: engine.sample_crps_weighted_tensor_ops(v, Sn, y, lw)},
        'quantiles': {'weighted': lambda v: engine.sample_quantiles(v, Sn, LEVELS, log_weight=lw),
                      'unweighted': lambda v: engine.sample_quantiles(v, Sn, LEVELS),
                      'ops': lambda v: engine.sample_quantiles_weighted_tensor_ops(v, Sn, LEVELS, lw)},
    }
    for name, variants in calls.items():
        with torch.no_grad():
            a, b = variants['weighted'](x), variants['ops'](x.double())
            a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
            say(f'{name:9s} weighted kernel against the float64 statement: max |difference| '
                f'{max(float((p.double() - q).abs().max()) for p, q in zip(a, b)):.3e}')
            fwd = alternate({k: (lambda f=f: f(x)) for k, f in variants.items()})
        both = alternate({k: (lambda f=f: torch.autograd.grad(total(f(xg)), xg)) for k, f in variants.items()})
        for k in variants:
            say(f'{name:9s} {k:10s} fwd     {fmt(fwd[k])}')
        for k in variants:
            say(f'{name:9s} {k:10s} fwd+bwd {fmt(both[k])}')
        m = lambda t, k: float(np.median(t[k]))
        say(f'{name:9s} weighted / unweighted: fwd {m(fwd, "weighted") / m(fwd, "unweighted"):.2f} x, fwd+bwd '
            f'{m(both, "weighted") / m(both, "unweighted"):.2f} x;  tensor ops / weighted: fwd {m(fwd, "ops") / m(fwd, "weighted"):.1f} x, '
            f'fwd+bwd {m(both, "ops") / m(both, "weighted"):.1f} x')
    del x, lw, y, xg
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
