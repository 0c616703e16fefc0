#!/usr/bin/env python
"""The bits of the unweighted energy score and its adjoint: tests/golden/sample_energy_bits.npz.

Recorded on the commit BEFORE the two energy kernels became one template (csrc/snsde_energy.hip), from engine.sample_energy and
engine.sample_energy_backward with neither weights nor mask; tests/test_gpu_sample_energy.py asserts torch.equal against it.  The
fixture holds the float32 inputs (seeded; in group 0 sample 1 duplicates sample 0, so a zero distance occurs) and the energy and
both gradients the kernels gave for them.

Cases: N on both sides of every bucket edge of the kernel - 2, 39 | 40, 87 | 88, 151 | 152, 256 - with G = 2 scores and V = 17 (a
16-column chunk and a tail of one); N = 88 once more as M = 2 members of S = 44; fair both ways at N = 40; one path=True case with
outer = 3, W = 7 (V = 21: a chunk straddles the outer axis).

Run from the repo root on a GPU against a built library:
  python tests/golden/make_sample_energy_bits.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

G, V = 2, 17
# name -> (outer or None, members, samples per member, width, fair, path)
CASES = {f'n{n}': (None, 1, n, V, True, False) for n in (2, 39, 40, 87, 88, 151, 152, 256)}
CASES['n40_unfair'] = (None, 1, 40, V, False, False)
CASES['n88_m2'] = (None, 2, 44, V, True, False)
CASES['path_o3_w7'] = (3, 1, 12, 7, True, True)


def inputs(index, outer, M, S, W, path):
    """ys (outer, M, G S, W) without the axes that are absent, target (outer, G, W), grad_energy (outer, G) or, under path, (G,)."""
    rng = np.random.default_rng(20240 + index)
    lead = () if outer is None else (outer,)
    x = (2.0 * rng.standard_normal(lead + (M, G, S, W)) + 0.5).astype(np.float32)
    x[..., 0, 0, 1, :] = x[..., 0, 0, 0, :]      # member 0, group 0: sample 1 = sample 0
    y = rng.standard_normal(lead + (G, W)).astype(np.float32)
    g = rng.standard_normal((G,) if path else lead + (G,)).astype(np.float32)
    x = x.reshape(lead + (M, G * S, W))
    return (x[..., 0, :, :] if M == 1 else x), y, g


def main():
    import torch
    from stable_neural_sdes_amd import engine
    out = {}
    for index, (name, (outer, M, S, W, fair, path)) in enumerate(CASES.items()):
        x, y, g = inputs(index, outer, M, S, W, path)
        xd, yd, gd = (torch.from_numpy(a).to('cuda:0') for a in (x, y, g))
        e = engine.sample_energy(xd, S, yd, fair=fair, members=M, path=path)
        gx, gy = engine.sample_energy_backward(gd, xd, yd, S, fair, M, path)
        assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all()), name
        out[f'{name}/cfg'] = np.array([M, S, int(fair), int(path)], np.int64)
        for key, a in (('x', x), ('y', y), ('g', g), ('energy', e.cpu().numpy()), ('gx', gx.cpu().numpy()), ('gy', gy.cpu().numpy())):
            out[f'{name}/{key}'] = a
        print(name, x.shape, 'energy', out[f'{name}/energy'].ravel()[:2])
    path_out = os.path.join(HERE, 'sample_energy_bits.npz')
    np.savez_compressed(path_out, **out)
    print(path_out, len(out), 'arrays,', os.path.getsize(path_out), 'bytes')


if __name__ == '__main__':
    main()
