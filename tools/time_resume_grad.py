#!/usr/bin/env python3
"""Training through continued solves: what the offset costs.  The K2 and K4 training legs of tools/time_configs.py
(forward + backward of one sdeint call, Philox increments regenerated in the adjoint) as one uncut call - the leg every earlier
measurement names, and the one to compare between two checkouts: the adjoints gained one uniform argument - and, where the
checkout has options={'resume_grad': True}, cut into two and four pieces chained through extra_solver_state.

HIP events around each training step, 5 warm-up steps, the median of 30; run it in alternating processes to compare two
checkouts (--root: the checkout whose package is imported, default this one):
    python tools/time_resume_grad.py [--root DIR] [--tag NAME] [output file to append to]"""
import os, sys
import numpy as np, torch
args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = 'this checkout'
while args and args[0] in ('--root', '--tag'):
    if args[0] == '--root':
        ROOT = os.path.abspath(args[1])
    else:
        tag = args[1]
    args = args[2:]
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from tests.helpers import make_problem
dev = torch.device('cuda:0')
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
    return f'median {np.median(v):9.1f} us  min {v.min():9.1f}  p90 {np.percentile(v, 90):9.1f}  ({len(v)} steps)'


has_resume = hasattr(S.engine, 'check_resume_grad')
say(f'# tools/time_resume_grad.py [{tag}]: forward + backward of one training step, HIP events, median of 30 after 5 warm-up steps')
CFG = [('K2 LNSDE', 4, 17, 2, 1024, 128, 21, 101, 'euler'), ('K4 NSDE sepsis-shaped', 3, 18, 2, 2048, 64, 69, 72, 'euler')]
for name, io, no, NL, B, H, C, L, method in CFG:
    pr = make_problem(7, io, no, NL, B, H, C, L, nan_frac=0.2)
    m = S.Diffusion_model(C, H, H, NL, input_option=io, noise_option=no)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(dev)
    times = torch.from_numpy(pr['times']).to(dev)
    m.set_X(torch.from_numpy(pr['coeffs']).to(dev), times)
    y0 = torch.from_numpy(pr['y0']).to(dev)
    N = L - 1

    def step(pieces):
        def run():
            m.zero_grad(set_to_none=True)
            yy = y0.clone().requires_grad_(True)
            if pieces == 1:
                ys = S.sdeint(m, yy, times[[0, -1]], method=method, dt=1.0, options={'seed': 1})
            else:
                cuts = [round(N * k / pieces) for k in range(pieces + 1)]
                y, state = yy, None
                for a, b in zip(cuts[:-1], cuts[1:]):
                    ys, state = S.sdeint(m, y, times[[a, b]], method=method, dt=1.0, options={'seed': 1, 'resume_grad': True}, extra=True,
                                         extra_solver_state=state)
                    y = ys[-1]
            ys[-1].square().mean().backward()
            return ys[-1].detach(), yy.grad
        return run

    whole = step(1)()
    for pieces in (1, 2, 4) if has_resume else (1,):
        fn = step(pieces)
        got = fn()
        event_ms(fn, 5)
        t = event_ms(fn, 30)
        note = '' if pieces == 1 else (f'   states equal the uncut call: {bool(torch.equal(got[0], whole[0]))}, max |dL/dy0 - uncut| '
                                       f'{float((got[1] - whole[1]).abs().max()):.2e} of {float(whole[1].abs().max()):.2e}')
        say(f'[{tag}] {name:22s} B={B} H={H} N={N} {method}: {pieces} piece{"s" if pieces > 1 else " "} fwd+bwd {fmt(t)}{note}')
if args:
    with open(args[0], 'a') as fh:
        fh.write('\n'.join(lines) + '\n')
