#!/usr/bin/env python
"""What the host layer's plan queries answer, and the descriptors they ask with: tests/golden/plans.npz.

Generated on the tree of commit 14d55e6 ("Opt-in training through wave-pair model ensembles"), the parent of the change that
moved every descriptor of stable-neural-sdes_amd/engine.py onto one configuration record (engine.SolveConfig).  The file pins
that tree's answers: tests/test_plan_config_cpu.py recomputes every row with the current engine and compares.  Regenerate it
only from a tree whose answers are meant to become the new reference, and name that commit here.

The grid (`grid()`; nothing of it is stored, the rows are in its order): six models x method x kernel x precision x members x
samples x batch x global_rows x eight masks of the six bool opt-ins x training planes, at 8 knots and 6 steps.  Per row
(`record()`): the indices of engine.forward_path, of engine.forward_kernel / engine.backward_kernel on engine.query_descriptor,
engine.backward_mode, and the descriptor's flags, members, samples, global_rows, method and kernel fields.  Only the engine's
public functions are called, with keywords, so the script runs unchanged on either side of that change.

Run from the repo root against a built library:  python tests/golden/make_plan_golden.py
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KNOTS, STEPS, C_ = 8, 6, 3
# (name, hidden_channels, hidden_hidden_channels, num_hidden_layers, input_option, noise_option)
MODELS = (('lean-64', 64, 64, 2, 4, 17), ('lean-128', 128, 128, 2, 4, 17), ('h256', 256, 256, 2, 4, 17), ('net-64', 64, 64, 2, 1, 18),
          ('net-128', 128, 128, 2, 1, 18), ('odd-48', 48, 48, 2, 4, 17))
METHODS = ('euler', 'milstein', 'srk')
KERNELS = ('auto', 'mfma4', 'mfma16', 'w4')
PRECISIONS = ('fp32', 'bf16')
MEMBERS = (0, 1, 3)
SAMPLES = (0, 1, 2)
BATCHES = (24, 2)
GLOBAL_ROWS = (0, 48)
OPT_INS = ('sample_grad', 'bf16_grad', 'ensemble_grad', 'ensemble_samples', 'ensemble_nets', 'ensemble_nets_grad')
MASKS = ((), ('sample_grad',), ('bf16_grad',), ('ensemble_grad',), ('ensemble_nets',), ('sample_grad', 'ensemble_grad', 'ensemble_samples'),
         ('ensemble_grad', 'ensemble_nets', 'ensemble_nets_grad'), OPT_INS)
TRAINING = (False, True)
COLUMNS = ('forward_path', 'forward_kernel', 'backward_kernel', 'backward_mode', 'flags', 'members', 'samples', 'global_rows', 'method',
           'kernel')


def grid():
    """The rows, as dicts: model (a MODELS entry), method, kernel, precision, members, samples, batch, global_rows, opt_ins (the
    set ones, a tuple of names) and training."""
    names = ('model', 'method', 'kernel', 'precision', 'members', 'samples', 'batch', 'global_rows', 'opt_ins', 'training')
    for row in itertools.product(MODELS, METHODS, KERNELS, PRECISIONS, MEMBERS, SAMPLES, BATCHES, GLOBAL_ROWS, MASKS, TRAINING):
        yield dict(zip(names, row))


def carriers(row):
    """The opt-ins of a row that mean something: sample_grad with samples > 1, the ensemble_* with members > 1 (ensemble_samples
    with both), bf16_grad with precision='bf16'."""
    has = {'sample_grad': row['samples'] > 1, 'bf16_grad': row['precision'] == 'bf16', 'ensemble_grad': row['members'] > 1,
           'ensemble_samples': row['members'] > 1 and row['samples'] > 1, 'ensemble_nets': row['members'] > 1,
           'ensemble_nets_grad': row['members'] > 1}
    return tuple(o for o in row['opt_ins'] if has[o])


def record(engine, row, host_grid, models):
    """COLUMNS of one row from the engine's public queries."""
    lib = engine._lib
    model = models[row['model'][0]]
    opts = {o: True for o in row['opt_ins']}
    common = dict(method=row['method'], kernel=row['kernel'], precision=row['precision'], global_rows=row['global_rows'],
                  samples=row['samples'], members=row['members'], **opts)
    path = engine.forward_path(model, row['batch'], KNOTS, STEPS, training=row['training'], **common)
    desc = engine.query_descriptor(model, row['batch'], KNOTS, STEPS, training=row['training'], **common)
    mode = engine.backward_mode(model, row['batch'], KNOTS, host_grid, **common)
    return (lib.PATHS.index(path), lib.FWD_KERNELS.index(engine.forward_kernel(desc)), lib.REV_KERNELS.index(engine.backward_kernel(desc)),
            mode, int(desc.flags), int(desc.members), int(desc.samples), int(desc.global_rows), int(desc.method), int(desc.kernel))


def host_grid(engine):
    """A host-only StepGrid of STEPS steps (engine.backward_mode reads its N and T)."""
    times = np.linspace(0.0, float(STEPS), KNOTS).astype(np.float32)
    g = engine.step_grid(np.array([0.0, float(STEPS)], np.float32), 1.0, times, None)
    assert g.N == STEPS
    return g


def table(engine, rows=None):
    """(n, len(COLUMNS)) int32: `record` of every row of `rows` (default: the whole grid)."""
    g = host_grid(engine)
    models = {m[0]: engine.model_struct(C_, m[1], m[2], m[3], m[4], m[5]) for m in MODELS}
    return np.array([record(engine, r, g, models) for r in (grid() if rows is None else rows)], np.int32)


def main():
    from stable_neural_sdes_amd import engine
    t = table(engine)
    out = os.path.join(HERE, 'plans.npz')
    np.savez_compressed(out, **{c: t[:, i].astype(np.int16 if np.abs(t[:, i]).max() < 2 ** 15 else np.int32) for i, c in enumerate(COLUMNS)})
    print(out, t.shape, os.path.getsize(out), 'bytes; paths:', np.bincount(t[:, 0], minlength=len(engine._lib.PATHS)).tolist(),
          'backward modes:', np.bincount(t[:, 3]).tolist())


if __name__ == '__main__':
    main()
