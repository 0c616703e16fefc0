#!/usr/bin/env python3
"""Training through the bf16-operand solve (options={'precision': 'bf16', 'bf16_grad': True}, DESIGN 3.1e "Training") against fp32
training, same process, HIP events, alternating blocks:
  * the whole sdeint + backward() call at K2 ((4,17) H = 128, C = 21, 1024 rows, 100 Euler steps, in-kernel Philox) and on the
    512-row K3 shard shape ((6,17) H = 128, C = 21, 200 steps, Hermite coefficients; half weight scale as in tests/bigcase.py, so
    that the adjoint stays finite in float32), 100 calls per variant in ten alternating blocks of ten;
  * the forward launch alone in training mode (act_save, traj kept; the prepare launch skipped), fp32 against bf16.

usage: python tools/time_bf16_grad.py [output file, default profiles/time_bf16_grad.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import make_problem
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'time_bf16_grad.txt')
lines = []
ON = {'precision': 'bf16', 'bf16_grad': True}


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


props = torch.cuda.get_device_properties(0)
say(f'# tools/time_bf16_grad.py: device name as the driver reports it "{props.name}", {getattr(props, "gcnArchName", "?")}, '
    f'{props.multi_processor_count} CUs; whole sdeint + backward() call and the training-mode forward launch,')
say('# fp32 against bf16 operands (bf16_grad), HIP events, ten alternating blocks of ten calls per variant')
for name, io, no, rows, L, kw in (('K2', 4, 17, 1024, 101, dict(nan_frac=0.3)),
                                  ('K3 shard', 6, 17, 512, 201, dict(nan_frac=0.0, hermite=True, weight_scale=0.5))):
    pr = make_problem(3, io, no, 2, rows, 128, 21, L, **kw)
    sde = S.Diffusion_model(21, 128, 128, 2, input_option=io, noise_option=no)
    sde.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in pr['params'].items()})
    sde = sde.to(dev)
    times = torch.from_numpy(pr['times']).to(dev)
    sde.set_X(torch.from_numpy(pr['coeffs']).to(dev), times)
    y0 = torch.from_numpy(pr['y0']).to(dev)
    ts = torch.tensor([0.0, float(L - 1)], device=dev)
    w = torch.randn(2, rows, 128, generator=torch.Generator().manual_seed(1)).to(dev)
    model, layout, numel = engine.recognise(sde)
    grid = engine.step_grid(np.array([0.0, float(L - 1)], np.float32), 1.0, pr['times'], dev)
    modes = (engine.backward_mode(model, rows, L, grid, 'euler'), engine.backward_mode(model, rows, L, grid, 'euler', precision='bf16', bf16_grad=True))
    say(f'## {name}: {rows} rows, {L - 1} Euler steps, io={io} no={no} H=128 NL=2 C=21; backward mode fp32 {modes[0]}, bf16_grad {modes[1]}')

    def step(opts):
        ys = S.sdeint(sde, y0, ts, method='euler', dt=1.0, options=dict(opts, seed=7))
        (ys * w).sum().backward()
        return ys

    fns = {'fp32 training': lambda: step({}), 'bf16_grad training': lambda: step(ON)}
    res = {}
    for k, f in fns.items():
        for _ in range(10):
            f()
        for p in sde.parameters():
            p.grad = None
        ys = f()
        torch.cuda.synchronize()
        res[k] = (ys.detach().double(), torch.cat([p.grad.reshape(-1) for p in sde.parameters()]).double())
    (ya, ga), (yb, gb) = res.values()
    say(f'bf16_grad vs fp32 (same Philox key): states relative L2 {float((yb - ya).norm() / ya.norm()):.3e}, flat parameter gradient relative L2 '
        f'{float((gb - ga).norm() / ga.norm()):.3e} (finite: {bool(torch.isfinite(gb).all())})')
    ms = {k: [] for k in fns}
    for _ in range(10):
        for k, f in fns.items():
            ms[k] += event_ms(f, 10)
    for k in fns:
        say(f'{k:28s} whole call      {fmt(ms[k])}')
    a, b = (float(np.median(v)) for v in ms.values())
    say(f'bf16_grad / fp32: whole call x{b / a:.3f} (median)')
    # the forward launch alone in training mode
    flat = engine.flatten_params(sde, layout, numel, dev)
    calls = {'fp32 training': engine.SolveCall(model, flat, sde.coeffs, grid, y0, seed=7, save_traj=True, save_act=True),
             'bf16_grad training': engine.SolveCall(model, flat, sde.coeffs, grid, y0, seed=7, save_traj=True, save_act=True, precision='bf16',
                                                    bf16_grad=True)}
    fw = {k: [] for k in calls}
    for c in calls.values():
        for _ in range(5):
            c.launch()
    torch.cuda.synchronize()
    for _ in range(10):
        for k, c in calls.items():
            fw[k] += event_ms(lambda: c.launch(reuse_prepared=True), 10)
    for k in calls:
        say(f'{k:28s} forward launch  {fmt(fw[k])}')
    a, b = (float(np.median(v)) for v in fw.values())
    say(f'bf16_grad / fp32: training-mode forward launch x{b / a:.3f} (median)')
open(out_path, 'w').write('\n'.join(lines) + '\n')
