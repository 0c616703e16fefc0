#!/usr/bin/env python3
"""Same-process A/B of the forward solve with f32 and with bf16 MFMA operands (SNSDE_FLAG_BF16_OPERANDS): K2 (Neural LNSDE
io=4 / no=17, 1024 rows, H = 128, 100 Euler steps) and, for the record, the 512-row K3 shard (Neural GSDE io=6 / no=17, H = 128,
200 steps, Hermite coefficients).  Kernel-only times (the prepare launch skipped: reuse_prepared) from HIP events, min and
median over several timed batches of launches, alternating the two precisions batch by batch; plus how far the bf16 states are
from the f32 ones under the same Philox key.  usage: python tools/time_bf16.py [out.txt]   """
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import stable_neural_sdes_amd as S  # noqa: E402

BATCHES, PER_BATCH, WARM = 7, 20, 5


def batch_us(call, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        call.launch(reuse_prepared=True)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def case(name, rows, io, no, n_steps, hermite, nan_frac):
    dev = torch.device('cuda:0')
    pr, _, flat, coeffs, y0 = bench.build_inputs(dev, 0, io=io, no=no, b=rows, l=n_steps + 1, nan_frac=nan_frac, hermite=hermite)
    model = S.engine.model_struct(bench.C, bench.H, bench.H, bench.NL, io, no)
    grid = S.engine.step_grid(np.array([0.0, float(n_steps)], np.float32), 1.0, pr['times'], dev)
    calls = {p: S.engine.SolveCall(model, flat, coeffs, grid, y0, seed=2024, precision=p) for p in ('fp32', 'bf16')}
    paths = {p: S.engine.forward_path(model, rows, pr['times'].shape[0], grid.N, precision=p) for p in calls}
    for c in calls.values():
        for _ in range(WARM):
            c.launch()
    torch.cuda.synchronize()
    mins, meds = {p: [] for p in calls}, {p: [] for p in calls}
    for _ in range(BATCHES):
        for p, c in calls.items():
            t = batch_us(c, PER_BATCH)
            mins[p].append(min(t))
            meds[p].append(float(np.median(t)))
    ys = {p: c.launch().double().cpu() for p, c in calls.items()}
    torch.cuda.synchronize()
    d = ys['bf16'] - ys['fp32']
    rel = float(d.norm() / ys['fp32'].norm())
    lines = [f'{name}: {rows} rows, {n_steps} steps, io={io} no={no} H={bench.H} NL={bench.NL} C={bench.C}']
    for p in calls:
        lines.append(f'  {p:4s} ({paths[p]:9s}) kernel us: min {min(mins[p]):7.1f}  median of batch medians {np.median(meds[p]):7.1f}'
                     f'  (batch medians {" ".join(f"{m:.1f}" for m in meds[p])})')
    ratio_min = min(mins['bf16']) / min(mins['fp32'])
    ratio_med = float(np.median(meds['bf16']) / np.median(meds['fp32']))
    lines.append(f'  bf16 / fp32: {ratio_min:.3f} (min), {ratio_med:.3f} (median)')
    lines.append(f'  bf16 vs fp32 states (same Philox key): relative L2 {rel:.3e}, max abs {float(d.abs().max()):.3e}')
    return lines


def main():
    out = []
    out += case('K2', 1024, 4, 17, 100, False, 0.3)
    out += case('K3 shard', 512, 6, 17, 200, True, 0.0)
    text = '\n'.join(out) + '\n'
    print(text, end='')
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write('# tools/time_bf16.py: ' + torch.cuda.get_device_name(0) + '\n' + text)


if __name__ == '__main__':
    main()
