"""The lean forward kernel's filler work spread over its operand-read windows (csrc/snsde_m4_kernel.h: LEAN_GPART_MODE,
LEAN_CARRY_MODE) moves instructions, not values: every case of tests/lean_windows_cases.py reproduces, bit for bit,
what the library of the commit before the change wrote on an MI355X (tests/golden/lean_windows.npz, recorded by
tests/golden/make_lean_windows.py): the states, and in training mode the trajectory, the increments and every (step, slot) plane of
the saved activations.  Each case asserts the kernel and the instantiation it ran (lean_windows_cases.run)."""
import os
import signal

import numpy as np
import pytest

from tests import lean_windows_cases as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lean_windows.npz')


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('lean windows GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case(golden):
    want = {'ys'}, {'ys', 'traj', 'dW_out', 'act_save_sha'}
    for name, c in W.CASES.items():
        assert {k.split('/')[1] for k in golden if k.split('/')[0] == name} == want[c.launch.train], name
    assert {k.split('/')[0] for k in golden} == set(W.CASES)


@pytest.mark.parametrize('name', list(W.CASES))
def test_outputs_are_bit_identical_to_the_recorded_ones(golden, name):
    got = W.run(name)
    c = W.CASES[name].launch
    assert got['ys'].shape == (len(c.ts), c.B, c.H) and np.isfinite(got['ys']).all()
    assert not np.array_equal(got['ys'][0], got['ys'][-1])      # (the solve moves)
    for key, val in got.items():
        ref = golden[f'{name}/{key}']
        assert val.shape == ref.shape and val.dtype == ref.dtype, (name, key)
        if not np.array_equal(val.view(np.uint8), ref.view(np.uint8)):
            planes = val.reshape((-1,) + val.shape[-2:]) != ref.reshape((-1,) + ref.shape[-2:])
            bad = np.flatnonzero(planes.reshape(planes.shape[0], -1).any(1))
            raise AssertionError(f'{name}/{key}: {int(planes.sum())} elements differ, first in plane {bad[0]} of {planes.shape[0]}')


def test_on_grid_schedules_agree_with_each_other(golden):
    # (a property of the fixture itself: the recorded schedules are one solve seen through different outputs)
    every = golden['every/ys']
    assert np.array_equal(golden['main_4_17/ys'][-1], every[-1])
    assert np.array_equal(golden['seventh/ys'], every[[int(t) for t in W.CASES['seventh'].launch.ts]])
    assert np.array_equal(golden['train_4_17/traj'][-1], golden['train_4_17/ys'][-1])
    assert np.array_equal(golden['general/ys'], golden['main_4_17/ys'])      # (tests/test_gpu_lean_spec.py: the two instantiations agree)
