#!/usr/bin/env python3
"""The adjoint of the resampling step: the fused backward kernel (snsde_sample_resample_backward) against the
backward of the same definition in tensor ops (autograd through engine.sample_resample_tensor_ops(differentiable=True)).  Same
process, HIP events, the variants alternating.

Shapes (B input rows, S paths per row, W state width): (1024, 8 | 32 | 128, 128) and (4096, 8, 64) - those of
tools/time_sample_resample.py; log-weights ~ N(0, 1) carried plus an increment, systematic resampling, threshold 0.5 and 1.
  fused     engine.sample_resample_backward on the forward's outputs (one launch, two allocations)
  ops       torch.autograd.grad through the graph of the tensor-op statement (the graph is built once, outside the timing)
"device" is the time per launch of twenty launches recorded into one graph and replayed: the kernel itself, and the bandwidth it
reaches against the 2 G S W 4 bytes of state gradient it reads and writes - the forward's traffic, whose figures stand in
profiles/sample_resample_ab.txt.
One training step of the filter: the K2 model ((4,17) H = 128, C = 21, L = 101), B = 256 input rows x S = 32 particles, 20
observations of 5 Euler steps each, a Gaussian likelihood of three state components: torchsde.sdeint_filter(differentiable=True)
and the backward of -logz[-1].mean(), with the fused resampling against the same driver with the tensor-op statement.

usage: python tools/time_sample_resample_grad.py [output file, default profiles/sample_resample_grad_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_resample_grad_ab.txt')
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


def graphed_us(fn, reps=20):
    """us per call of `reps` calls recorded into one graph and replayed (ten replays, the median)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(reps)]
    graph.replay()
    t = event_ms(graph.replay, 10)
    del graph, keep
    return float(np.median(t)) * 1e3 / reps


def alternate(fns, blocks=8, per=5):
    t = {k: [] for k in fns}
    for f in fns.values():
        event_ms(f, 3)
    for _ in range(blocks):
        for k, f in fns.items():
            t[k] += event_ms(f, per)
    return t


say('# tools/time_sample_resample_grad.py: gradients of state (B S, W), log_weight (B, S) and logz (B,) on the device, float32; HIP events,')
say('# variants alternating in one process (eight blocks of five calls each); slower = a shape at which the kernel loses to autograd')
slower = []
for B, Sn, W in ((1024, 8, 128), (1024, 32, 128), (1024, 128, 128), (4096, 8, 64)):
    gen = torch.Generator().manual_seed(Sn + W)
    x = torch.randn(B * Sn, W, generator=gen).to(dev)
    lw, inc = torch.randn(B, Sn, generator=gen).to(dev), torch.randn(B, Sn, generator=gen).to(dev)
    u = torch.rand(B, generator=gen).to(dev)
    gs, gl, gz = torch.randn(B * Sn, W, generator=gen).to(dev), torch.randn(B, Sn, generator=gen).to(dev), torch.randn(B, generator=gen).to(dev)
    moved = 2 * x.numel() * 4
    say(f'## (B, S, W) = ({B}, {Sn}, {W}): {B} groups, state gradient {x.numel() * 4 / 2 ** 20:.2f} MiB, {moved / 2 ** 20:.2f} MiB read + written')
    for thr in (0.5, 1.0):
        with torch.no_grad():
            fwd = engine.sample_resample(x, Sn, lw, inc, u, thr)
        leaves = [t.clone().requires_grad_(True) for t in (x, lw, inc)]
        ops = engine.sample_resample_tensor_ops(leaves[0], Sn, leaves[1], leaves[2], u, thr, differentiable=True)
        same = bool(torch.equal(ops.ancestor, fwd.ancestor))
        fns = {'fused': lambda: engine.sample_resample_backward(gs, gl, gz, lw, inc, fwd.ancestor, fwd.resampled, Sn),
               'ops': lambda: torch.autograd.grad([ops.state, ops.log_weight, ops.logz], leaves, [gs, gl, gz], retain_graph=True)}
        a, b = fns['fused'](), fns['ops']()
        say(f'threshold {thr}: rows resampled {int(fwd.resampled.sum())} of {B}; ancestors of the two forwards equal: {same};  '
            f'max |grad_state fused - ops| {float((a[0] - b[0]).abs().max()):.3e}   max |grad_a fused - ops| {float((a[1] - b[1]).abs().max()):.3e}')
        t = alternate(fns)
        for k in fns:
            say(f'threshold {thr}: {k:6s} {fmt(t[k])}')
        d = graphed_us(fns['fused'])
        say(f'threshold {thr}: device fused {d:7.1f} us per launch (twenty in one graph), {moved / d / 1e3:.0f} GB/s of state gradient read + written')
        r = np.median(t['ops']) / np.median(t['fused'])
        say(f'threshold {thr}: fused backward against autograd through the tensor-op statement {r:.1f} x')
        if r < 1.0:
            slower.append((B, Sn, W, thr))
        del ops, leaves, fwd
    del x, lw, inc, u, gs, gl, gz
    torch.cuda.empty_cache()

# one training step of the filter
B, Sn, T, per = 256, 32, 20, 5
sde, times, _ = bench._module(dev, bench.IO, bench.NO, B, bench.H, bench.C, bench.L, 3)
sde.requires_grad_(True)
ts = torch.arange(0, T * per + 1, per, dtype=torch.float32, device=dev)
y0 = (0.5 * torch.randn(B, bench.H, generator=torch.Generator().manual_seed(5))).to(dev)
obs = torch.zeros(B, 3, device=dev)
like = lambda k, yk: engine.sample_loglik(yk[:, :3].contiguous(), Sn, obs, std=0.5, stats=True)[1]
opts = {'samples': Sn, 'seed': 11}
fused_step = engine.sample_resample


def train_step(step):
    def run():      # (the driver calls engine.sample_resample: the A/B swaps the name for the duration of the call)
        engine.sample_resample = step
        try:
            r = S.sdeint_filter(sde, y0, ts, like, method='euler', dt=1.0, options=opts, generator=torch.Generator(dev).manual_seed(1),
                                differentiable=True)
        finally:
            engine.sample_resample = fused_step
        sde.zero_grad(set_to_none=True)
        loss = -r.logz[-1].mean()
        loss.backward()
        return loss.detach(), [p.grad for p in sde.parameters()]
    return run


steps = {'fused': train_step(fused_step), 'ops': train_step(engine.sample_resample_tensor_ops)}
say(f'## filter training step: K2 model (io={bench.IO}, no={bench.NO}, H={bench.H}, C={bench.C}, L={bench.L}), B = {B} x S = {Sn} particles, {T} '
    f'observations of {per} Euler steps each: sdeint_filter(differentiable=True) and the backward of -logz[-1].mean()')
got = {k: f() for k, f in steps.items()}
worst = max(float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30) for a, b in zip(got['fused'][1], got['ops'][1]))
say(f'loss fused / ops {float(got["fused"][0]):.4f} / {float(got["ops"][0]):.4f};  largest parameter-gradient difference relative to the tensor\'s '
    f'largest entry {worst:.3e}')
t = alternate(steps, blocks=5, per=3)
for k in steps:
    say(f'filter training step {k:6s} {fmt(t[k])}')
r = np.median(t['ops']) / np.median(t['fused'])
say(f'filter training step: the driver with the fused resampling against the driver with the tensor-op statement {r:.2f} x '
    f'({(np.median(t["ops"]) - np.median(t["fused"])) * 1e3 / T:.1f} us per observation)')
if r < 1.0:
    slower.append('filter training step')
say(f'# shapes at which the fused route is slower than the statement: {slower if slower else "none"}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
