#!/usr/bin/env python3
"""Particle filtering on sample paths: the fused weigh-and-resample kernel (snsde_sample_resample) against the
same definition in tensor ops (engine.sample_resample_tensor_ops).  Same process, HIP events, the variants alternating.

Shapes (B input rows, S paths per row, W state width): (1024, 8 | 32 | 128, 128) and (4096, 8, 64); log-weights ~ N(0, 1) carried
plus an increment, systematic resampling, threshold 0.5 (about half of the rows resample) and threshold 1 (all of them).
  fused     engine.sample_resample on CUDA float32 (one launch)
  ops       engine.sample_resample_tensor_ops (logsumexp, exp, cumsum, searchsorted, gather, where, ...)
The event times of the fused route are mostly host time (one launch behind a Python call that allocates six outputs); "device" is
the time per launch of twenty launches recorded into one graph and replayed: the kernel itself, and the bandwidth it reaches
against the 2 G S W 4 bytes of state it must read and write.
One filter loop: the K2 model ((4,17) H = 128, C = 21, L = 101), B = 256 input rows x S = 32 particles, 20 observations of 5 Euler
steps each, a Gaussian likelihood of three state components (sample_loglik): torchsde.sdeint_filter with the kernel against the
same driver with the tensor-op statement.

usage: python tools/time_sample_resample.py [output file, default profiles/sample_resample_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
import bench
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_resample_ab.txt')
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


say('# tools/time_sample_resample.py: state (B S, W) float32, log_weight and log_increment (B, S), u (B,) on the device; HIP events, variants')
say('# alternating in one process (eight blocks of five calls each); slower = a shape at which the kernel loses to the statement')
slower = []
with torch.no_grad():
    for B, Sn, W in ((1024, 8, 128), (1024, 32, 128), (1024, 128, 128), (4096, 8, 64)):
        gen = torch.Generator().manual_seed(Sn + W)
        x = torch.randn(B * Sn, W, generator=gen).to(dev)
        lw, inc = torch.randn(B, Sn, generator=gen).to(dev), torch.randn(B, Sn, generator=gen).to(dev)
        u = torch.rand(B, generator=gen).to(dev)
        moved = 2 * x.numel() * 4
        say(f'## (B, S, W) = ({B}, {Sn}, {W}): {B} groups, state {x.numel() * 4 / 2 ** 20:.2f} MiB, {moved / 2 ** 20:.2f} MiB read + written')
        for thr in (0.5, 1.0):
            fns = {'fused': lambda: engine.sample_resample(x, Sn, lw, inc, u, thr), 'ops': lambda: engine.sample_resample_tensor_ops(x, Sn, lw, inc, u, thr)}
            got = {k: f() for k, f in fns.items()}
            ref = engine.sample_resample_tensor_ops(x.double(), Sn, lw.double(), inc.double(), u.double(), thr)
            for k, g in got.items():
                say(f'threshold {thr}: {k:6s} ancestors that differ from the float64 statement {int((g.ancestor != ref.ancestor).sum())} of {B * Sn}'
                    f'   max |logz - float64| {float((g.logz.double() - ref.logz).abs().max()):.3e}   rows resampled {int(g.resampled.sum())} of {B}')
            t = alternate(fns)
            for k in fns:
                say(f'threshold {thr}: {k:6s} {fmt(t[k])}')
            d = graphed_us(fns['fused'])
            say(f'threshold {thr}: device fused {d:7.1f} us per launch (twenty in one graph), {moved / d / 1e3:.0f} GB/s of state read + written')
            r = np.median(t['ops']) / np.median(t['fused'])
            say(f'threshold {thr}: fused against the tensor-op statement {r:.1f} x')
            if r < 1.0:
                slower.append((B, Sn, W, thr))
        del x, lw, inc, u
        torch.cuda.empty_cache()

    # one filter loop
    B, Sn, T, per = 256, 32, 20, 5
    sde, times, _ = bench._module(dev, bench.IO, bench.NO, B, bench.H, bench.C, bench.L, 3)
    ts = torch.arange(0, T * per + 1, per, dtype=torch.float32, device=dev)
    y0 = (0.5 * torch.randn(B, bench.H, generator=torch.Generator().manual_seed(5))).to(dev)
    obs = torch.zeros(B, 3, device=dev)
    like = lambda k, yk: engine.sample_loglik(yk[:, :3].contiguous(), Sn, obs, std=0.5, stats=True)[1]
    opts = {'samples': Sn, 'seed': 11}
    fused_step = engine.sample_resample

    def loop(step):
        def run():      # (the driver calls engine.sample_resample: the A/B swaps the name for the duration of the call)
            engine.sample_resample = step
            try:
                return S.sdeint_filter(sde, y0, ts, like, method='euler', dt=1.0, options=opts, generator=torch.Generator(dev).manual_seed(1))
            finally:
                engine.sample_resample = fused_step
        return run
    loops = {'fused': loop(fused_step), 'ops': loop(engine.sample_resample_tensor_ops)}
    say(f'## filter loop: K2 model (io={bench.IO}, no={bench.NO}, H={bench.H}, C={bench.C}, L={bench.L}), B = {B} x S = {Sn} particles, {T} observations of {per} '
        f'Euler steps each, whole sdeint_filter call')
    got = {k: f() for k, f in loops.items()}
    say(f'rows resampled per observation (fused): {[int(v) for v in (got["fused"].ess[1:] < 0.5 * Sn).sum(1).tolist()]} of {B};  '
        f'final logz fused / ops mean {float(got["fused"].logz[-1].mean()):.4f} / {float(got["ops"].logz[-1].mean()):.4f}')
    t = alternate(loops, blocks=5, per=3)
    for k in loops:
        say(f'filter loop {k:6s} {fmt(t[k])}')
    r = np.median(t['ops']) / np.median(t['fused'])
    say(f'filter loop: the driver with the kernel against the driver with the tensor-op statement {r:.2f} x '
        f'({(np.median(t["ops"]) - np.median(t["fused"])) * 1e3 / T:.1f} us per observation)')
    if r < 1.0:
        slower.append('filter loop')
say(f'# shapes at which the fused route is slower than the statement: {slower if slower else "none"}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
