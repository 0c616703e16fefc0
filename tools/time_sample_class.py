#!/usr/bin/env python3
"""Classification with sample paths: the fused kernels (snsde_sample_class / _backward) against the same
definition in tensor ops.  Same process, HIP events, the variants alternating; time and peak allocated memory.

Shapes (B input rows, S paths per row, C classes):
  (1024, 8 | 32 | 128, 35)   Speech Commands' 35 classes at the sample counts of the other score files
  (4096, 8, 10)              a large batch of a ten-class task
  (1024, 32, binary)         the sepsis task: one logit per path, class_weight = (1, pos_weight)
  (256, 16, 1000)            a wide head: the 256-column sweep, the slab still staged in LDS
  fused     engine.sample_class on CUDA float32 (one launch forward, one backward)
  ops       engine.sample_class_tensor_ops, autograd for the backward
forward alone (no_grad, stats=True: nll, xent, logp, probs and the entropies) and forward + backward (dL/d logits of the mean nll).
The event times of the fused route are mostly host time (one launch behind a Python call that allocates six outputs); "device"
is the time per launch of twenty launches recorded into one graph and replayed: the kernels themselves.

usage: python tools/time_sample_class.py [output file, default profiles/sample_class_ab.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
dev = torch.device('cuda:0')
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sample_class_ab.txt')
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


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


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
        event_ms(f, 2)
    for _ in range(blocks):
        for k, f in fns.items():
            t[k] += event_ms(f, per)
    return t


say('# tools/time_sample_class.py: logits (B S, C) float32, labels (B,) int64, log_weight (B, S), class_weight (C); binary: logits (B S, 1);')
say('# HIP events, variants alternating in one process (eight blocks of five calls each); slower = a shape at which the kernel loses to the statement')
slower = []
for B, Sn, Cn in ((1024, 8, 35), (1024, 32, 35), (1024, 128, 35), (4096, 8, 10), (1024, 32, 0), (256, 16, 1000)):
    binary = Cn == 0
    W, classes = (1, 2) if binary else (Cn, Cn)
    gen = torch.Generator().manual_seed(Sn + Cn)
    z = (2.0 * torch.randn(B * Sn, W, generator=gen)).to(dev)
    y = torch.randint(0, classes, (B,), generator=gen).to(dev)
    lw = (0.1 * torch.randn(B, Sn, generator=gen)).to(dev)
    cw = (0.5 + torch.rand(classes, generator=gen)).to(dev)
    zg = z.clone().requires_grad_(True)
    kw = dict(binary=binary, log_weight=lw, class_weight=cw)
    fwd = {'fused': lambda: S.sample_class(z, Sn, y, stats=True, **kw), 'ops': lambda: engine.sample_class_tensor_ops(z, Sn, y, stats=True, **kw)}

    def train(f):
        def run():
            zg.grad = None
            f(zg).mean().backward()
        return run
    bwd = {'fused': train(lambda a: S.sample_class(a, Sn, y, **kw)), 'ops': train(lambda a: engine.sample_class_tensor_ops(a, Sn, y, **kw))}
    say(f'## (B, S, C) = ({B}, {Sn}, {"binary" if binary else Cn}): N = {Sn}, {B} groups, logits {z.numel() * 4 / 2 ** 20:.2f} MiB')
    ref = engine.sample_class_tensor_ops(z.double(), Sn, y, stats=True, binary=binary, log_weight=lw.double(), class_weight=cw.double())
    with torch.no_grad():
        for k, f in fwd.items():
            got = f()
            say(f'{k:6s} max |nll - float64 statement| {float((got.nll.double() - ref.nll).abs().max()):.3e} (nll ~ {float(ref.nll.mean()):.2f})'
                f'   max |mutual information - float64| {float((got.mutual_information.double() - ref.mutual_information).abs().max()):.3e}'
                f' (~ {float(ref.mutual_information.mean()):.3f})')
        tf = alternate(fwd)
        mf = {k: peak_mb(f) for k, f in fwd.items()}
    tb = alternate(bwd)
    mb = {k: peak_mb(f) for k, f in bwd.items()}
    for k in fwd:
        say(f'forward            {k:6s} {fmt(tf[k])}   peak {mf[k]:9.1f} MiB')
    for k in bwd:
        say(f'forward + backward {k:6s} {fmt(tb[k])}   peak {mb[k]:9.1f} MiB')
    gn = torch.full((B,), 1.0 / B, device=dev)
    with torch.no_grad():
        df = graphed_us(lambda: S.sample_class(z, Sn, y, stats=True, **kw))
        db = graphed_us(lambda: engine.sample_class_backward(gn, None, None, z, Sn, y, grad_log_weight=False, **kw))
    say(f'device             fused  forward {df:7.1f} us  backward {db:7.1f} us per launch (twenty in one graph), '
        f'{z.numel() * 4 / df / 1e3:.0f} / {2 * z.numel() * 4 / db / 1e3:.0f} GB/s of logits read, and read + written')
    rf, rb = np.median(tf['ops']) / np.median(tf['fused']), np.median(tb['ops']) / np.median(tb['fused'])
    say(f'fused against the tensor-op statement: forward {rf:.1f} x, forward + backward {rb:.1f} x')
    if rf < 1.0 or rb < 1.0:
        slower.append((B, Sn, Cn))
    del z, y, zg, ref, lw
    torch.cuda.empty_cache()
say(f'# shapes at which the fused route is slower than the statement: {slower if slower else "none"}')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
