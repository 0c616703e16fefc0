"""Host side of the inference-stream tests (tests/test_inference_stream_cpu.py, tests/test_gpu_inference_stream.py): the stream
coordinates, the specified increments at those coordinates and the oracle pair on a set of increments.  Plain numpy on
oracle/sde_oracle.py; importable without a GPU.

The cases are tests/kernel_cases.py:STEP_OFFSET_CASES (every forward kernel once, 37 steps of dt = 0.25) on the inputs of
tests/test_gpu_step_offset.py (make_problem seed 21, Philox key SEED, row_offset 40)."""
from collections import namedtuple

import numpy as np

from oracle import sde_oracle as O
from tests.helpers import make_problem
from tests.kernel_cases import STEP_OFFSET_CASES

CASES = STEP_OFFSET_CASES
PROBLEM_SEED = 21                      # tests/test_gpu_step_offset.py:_Problem
SEED = 0x0123_4567_89AB_CDEF           # tests/test_gpu_step_offset.py
ROW_OFFSET = 40
N_STEPS = 37
MAX_STEP_OFFSET = 2 ** 31 - 1 - N_STEPS      # the last global step is INT32_MAX - 1 (include/snsde.h: snsde_solve_forward_at)

Coords = namedtuple('Coords', 'name seed row_offset step_offset')


def max_row_offset(B):
    """The last legal rows: row_offset + B = 2^32 (include/snsde.h: snsde_solve.row_offset)."""
    return 2 ** 32 - B


def coordinate_sets(c):
    """The stream coordinates a case is run at: the coordinates of tests/test_gpu_step_offset.py, a second pass at step_offset = 6
    (phase 2 of a Philox block, a piece of the first 16-step batch of the lean kernel), one combined extreme - and, for two cases, every
    coordinate moved alone: each key half on its own, rows across the int32 sign bit, a small odd and the largest step offset."""
    out = [Coords('base', SEED, ROW_OFFSET, 0), Coords('step 6', SEED, ROW_OFFSET, 6),
           Coords('extreme', 2 ** 64 - 1, max_row_offset(c.B), MAX_STEP_OFFSET)]
    if c.test in ('lean general', 'generic srk'):
        out += [Coords(f'seed {s:#x}', s, ROW_OFFSET, 0) for s in (0, 0xFFFFFFFF, 1 << 32)]
        out += [Coords('rows over 2^31', SEED, 2 ** 31 - 4, 0)]
        out += [Coords('step 3', SEED, ROW_OFFSET, 3), Coords('last steps', SEED, ROW_OFFSET, MAX_STEP_OFFSET)]
    return out


def problem(c):
    return make_problem(PROBLEM_SEED, c.io, c.no, c.NL, c.B, c.H, c.C, c.L)


def step_times(c):
    t0, t1, *_ = O.step_grid(np.asarray(c.ts, np.float32), c.dt)
    assert len(t0) == N_STEPS
    return t0, t1


def specified_increments(c, seed, row_offset, step_offset=0, rows=None, cols=None):
    """(dW, dU) the specification draws for the case at these coordinates, (N, B, H) float32 each (dU: SRK only, else None) - built as
    tests/test_gpu_step_offset.py:test_the_offset_draws_the_specified_stream builds its expectation: local step n is global step
    step_offset + n; at offset 0 these are O.philox_dW / O.philox_dU.  rows / cols: other global rows / a column window (start, stop) of
    a wider stream - what the shifted-stream tests pass."""
    t0, t1 = step_times(c)
    rows = np.arange(row_offset, row_offset + c.B) if rows is None else rows
    lo, hi = (0, c.H) if cols is None else cols
    h = (t1 - t0).astype(np.float32)
    dW = np.stack([O.philox_normals(seed, rows, step_offset + n, hi)[:, lo:] * np.sqrt(h[n], dtype=np.float32) for n in range(len(h))])
    if c.method != 'srk':
        return dW, None
    xi = np.stack([O.philox_normals(seed, rows, step_offset + n, hi, stream=1)[:, lo:] for n in range(len(h))])
    hh = h[:, None, None]
    return dW, hh * (np.float32(0.5) * dW + np.sqrt(hh / np.float32(12), dtype=np.float32) * xi)


def oracle_states(pr, c, dW, dU, dtype):
    """The output states of the case on these increments (tests/test_gpu_parity.py: oracle_solve, test_srk_trajectory_vs_oracle)."""
    return O.solve_diffusion_model(pr['params'], c.io, c.no, pr['coeffs'], pr['times'], pr['y0'], np.asarray(c.ts, np.float32), c.dt, dW,
                                   method=c.method, dtype=dtype, dU=dU)[0]


def one_ulp_up(x):
    """Every element moved by one float32 ulp (towards +inf)."""
    return None if x is None else np.nextafter(x, np.float32(np.inf), dtype=np.float32)
