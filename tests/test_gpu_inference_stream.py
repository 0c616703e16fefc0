"""The Brownian stream of inference-mode solves, on every forward kernel (DESIGN sections 1 and 4).

A solve that draws its increments in the kernel and writes no dW_out is a compiled kernel of its own (SAVE = 0; for K2 the lean
specialised one).  Each case of tests/kernel_cases.py:STEP_OFFSET_CASES - every forward kernel once - is tied to the stream
specification (oracle/sde_oracle.py:philox_normals) by one chain:

  a. the increments D the training-mode launch of the same case WRITES at these coordinates are the specified ones
     (O.philox_dW / O.philox_dU, rtol 2e-6, atol 2e-7);
  b. the inference launch (no saved plane, no supplied increment) runs the kernel - and the lean variant - the case names;
  c. its states pass the parity criterion (tests/helpers.py:assert_parity, SURVEY 8c, unchanged) against the float64 oracle ON D:
     tests/test_inference_stream_cpu.py shows that the float32 oracle sits two orders of magnitude inside that criterion on the
     right stream and more than three outside it one column, one row or one step off;
  d. they equal, bit for bit, the inference launch of the same case with D supplied: both hand the same float to the same arithmetic.

The coordinates: those of tests/test_gpu_step_offset.py, a second pass at step_offset = 6, the combined extreme (all key bits set,
the last legal rows, the last legal steps) and, for the lean general and the generic SRK case, each coordinate moved alone.

Step (d) holds bit for bit on every kernel at every coordinate set measured (profiles/inference_stream_margins.txt): every kernel
rounds z * sqrt(h) to a float before it enters the update, as the written plane holds it, so no family needs a looser replay bound
and none is given one.

With SNSDE_STREAM_MARGINS set to a file name every chain appends its measured figures to it (profiles/inference_stream_margins.txt
is such a run)."""
import os

import numpy as np
import pytest
import torch

from stable_neural_sdes_amd import engine
from tests import inference_stream as IS
from tests.bf16_reference import solve_bf16
from tests.helpers import assert_kernels, assert_parity, param_spec, parity_report

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

CASES = IS.CASES
LEAN_VARIANT = {'lean specialised': 'specialised', 'lean general': 'general', 'lean general milstein': 'general'}      # (test_gpu_step_offset.py)
# with supplied increments the specialised lean kernel is not planned (csrc/snsde_mfma.hip: make_plan specialises only where the solve
# draws its own increments), so the replay of that case runs the general instantiation - by construction, and tests/test_gpu_lean_spec.py
# holds the two to the same bits under the same key
REPLAY_VARIANT = dict(LEAN_VARIANT, **{'lean specialised': 'general'})
RTOL, ATOL = 2e-6, 2e-7      # written increments against the specification: the project's figure (test_philox_increments_match_specification)


class _Problem:
    """The device inputs of a case, built once; call(coords, **kw) describes one solve on them at those stream coordinates."""

    def __init__(self, c):
        self.c = c
        self.pr = pr = IS.problem(c)
        self.model = engine.model_struct(c.C, c.H, c.H, c.NL, c.io, c.no)
        spec = param_spec(c.io, c.no, c.NL, c.C, c.H)
        self.flat = torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in spec])).to(DEV)
        self.coeffs, self.y0 = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['y0']).to(DEV)
        self.grid = engine.step_grid(np.array(c.ts, np.float32), c.dt, pr['times'], torch.device(DEV))
        t0, t1 = IS.step_times(c)
        assert np.array_equal(self.grid.t0, t0) and np.array_equal(self.grid.t1, t1)

    def call(self, coords, seed=None, **kw):
        c = self.c
        kw = dict(dict(method=c.method, kernel=c.kernel, stream_all=c.stream_all, two_tile=c.two_tile, exact_order=c.exact,
                       precision='bf16' if c.bf16 else 'fp32'), **kw)
        return engine.SolveCall(self.model, self.flat, self.coeffs, self.grid, self.y0, seed=coords.seed if seed is None else seed,
                                row_offset=coords.row_offset, step_offset=coords.step_offset, **kw)


_PROBLEMS = {}


def _problem(c):
    if c.test not in _PROBLEMS:
        _PROBLEMS[c.test] = _Problem(c)
    return _PROBLEMS[c.test]


def _note(line):
    if os.environ.get('SNSDE_STREAM_MARGINS'):
        with open(os.environ['SNSDE_STREAM_MARGINS'], 'a') as fh:
            fh.write(line + '\n')


def _assert_written(got, exp, what):
    """A written plane against the specification; returns the worst relative error (over the elements above atol / rtol, where the
    relative term of the tolerance is the larger one)."""
    err = np.abs(got.astype(np.float64) - exp)
    big = np.abs(exp) >= ATOL / RTOL
    worst = float((err[big] / np.abs(exp[big])).max())
    print(what, 'worst relative error', worst, 'worst error in units of the tolerance', float((err / (ATOL + RTOL * np.abs(exp))).max()))
    np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL, err_msg=what)
    return worst


def _reference(p, dW, dU):
    """(ref64, cpu32) of the case on these increments; the bf16 case: the float64 restatement with the kernel's operand rounding."""
    c = p.c
    if c.bf16:
        return solve_bf16(p.pr['params'], c.io, c.no, p.pr['coeffs'], p.pr['times'], p.pr['y0'], np.asarray(c.ts, np.float32), c.dt, dW,
                          method=c.method)[0], None
    return IS.oracle_states(p.pr, c, dW, dU, np.float64), IS.oracle_states(p.pr, c, dW, dU, np.float32)


def _chain(c, coords):
    p = _problem(c)
    what = f'{c.test} @ {coords.name}'
    # a. the written increments are the specified ones.  The bf16 kernel has no training-mode route without bf16_grad: its D comes from
    #    the generic kernel at the same coordinates (tests/test_inference_stream_cpu.py holds every other case to its own kernel there)
    written = p.call(coords, save_dW=True, **(dict(kernel='generic', precision='fp32') if c.bf16 else {}))
    assert_kernels(written, fwd='generic' if c.bf16 else c.fwd)
    written.launch()
    D = written.dW_out.clone()
    dU = written.dU_out.clone() if c.method == 'srk' else None
    dW_h, dU_h = D.cpu().numpy(), None if dU is None else dU.cpu().numpy()
    exp_W, exp_U = IS.specified_increments(c, coords.seed, coords.row_offset, coords.step_offset)
    worst = _assert_written(dW_h, exp_W, f'{what}: dW_out')
    if dU is not None:
        worst = max(worst, _assert_written(dU_h, exp_U, f'{what}: dU_out'))
    # b. the inference launch: no saved plane, no supplied increment
    phx = p.call(coords)
    assert_kernels(phx, fwd=c.fwd)
    assert phx.dW_out is None and phx.traj is None and phx.act_save is None
    if c.test in LEAN_VARIANT:
        assert engine.lean_variant(phx) == LEAN_VARIANT[c.test]
    ys_phx = phx.launch().clone()
    got = ys_phx.cpu().numpy()
    # c. the arbiter on identical increments
    ref64, cpu32 = _reference(p, dW_h, dU_h)
    if c.bf16:      # the bounds of tests/test_gpu_bf16.py:test_states_match_the_bf16_reference
        assert np.isfinite(got).all()
        rel, worst_abs = float(np.linalg.norm(got - ref64) / np.linalg.norm(ref64)), float(np.abs(got - ref64).max())
        bound_abs = 1e-3 * max(1.0, float(np.abs(ref64).max()))
        print(what, 'relative L2', rel, 'max abs', worst_abs, 'bound', bound_abs)
        figures = f'rel_l2 {rel:.3e} (<= 1e-4) max {worst_abs:.3e} (<= {bound_abs:.3e})'
    else:
        rep = parity_report(got, ref64, cpu32)
        print(what, rep)
        figures = (f"mean {rep['mean']:.3e} (<= 1e-5, <= 4 cpu + 1e-7 = {4 * rep['cpu_mean'] + 1e-7:.3e}) max {rep['max']:.3e} (<= 5e-3, <= 4 cpu + 1e-6 = "
                   f"{4 * rep['cpu_max'] + 1e-6:.3e}) frac_ok {rep['frac_ok']:.6f} (>= 0.9999)")
    # d. the replay: the same case on D supplied, inference mode
    sup = p.call(coords, dW=D, dU=dU)
    assert_kernels(sup, fwd=c.fwd)
    if c.test in REPLAY_VARIANT:
        assert engine.lean_variant(sup) == REPLAY_VARIANT[c.test]
    ys_sup = sup.launch()
    equal = torch.equal(ys_phx, ys_sup)
    diff = float((ys_phx - ys_sup).abs().max())
    _note(f'{c.test:22s} {coords.name:16s} {c.fwd:19s} {figures} | dW_out worst rel {worst:.2e} | replay '
          f"{'bit-equal' if equal else f'max diff {diff:.3e}'}")
    if c.bf16:
        assert rel <= 1e-4 and worst_abs <= bound_abs, (what, rel, worst_abs)
    else:
        assert_parity(got, ref64, cpu32, what=what)
    assert equal, (what, 'the replay of the written increments differs by', diff)
    return ys_phx


@pytest.mark.parametrize('case', CASES, ids=[c.test for c in CASES])
def test_inference_solves_integrate_the_specified_stream(case):
    for coords in IS.coordinate_sets(case)[:2]:      # the coordinates of tests/test_gpu_step_offset.py, and a second pass at step_offset = 6
        _chain(case, coords)


@pytest.mark.parametrize('case', CASES, ids=[c.test for c in CASES])
def test_the_extreme_coordinates(case):
    """All 64 key bits set, the last legal rows (row_offset + B = 2^32) and the last legal steps (the last global step is INT32_MAX - 1)
    together: the same chain, no new shapes."""
    coords = IS.coordinate_sets(case)[2]
    assert (coords.seed, coords.row_offset + case.B, coords.step_offset + IS.N_STEPS) == (2 ** 64 - 1, 2 ** 32, 2 ** 31 - 1)
    _chain(case, coords)


SINGLE = [(c, k) for c in CASES for k in IS.coordinate_sets(c)[3:]]


@pytest.mark.parametrize('case,coords', SINGLE, ids=[f'{c.test}-{k.name}' for c, k in SINGLE])
def test_each_coordinate_alone(case, coords):
    """Each key half alone, rows across the int32 sign bit, an odd and the largest step offset - on one MFMA and one generic kernel."""
    assert case.test in ('lean general', 'generic srk')
    _chain(case, coords)


def test_each_coordinate_alone_is_run_on_both_families():
    assert sorted({c.test for c, _ in SINGLE}) == ['generic srk', 'lean general'] and len(SINGLE) == 12


@pytest.mark.parametrize('test', ['lean specialised', 'w4 euler', 'generic euler'])
def test_a_device_resident_key_draws_the_bits_of_the_integer_key(test):
    """seed as a one-element int64 CUDA tensor holding the same 64 bits (negative where the high bit is set): the inference launch
    reads the key from memory (snsde_solve.seed_dev) and must draw what the integer key draws."""
    case = next(c for c in CASES if c.test == test)
    p = _problem(case)
    outs = []
    for key in (IS.SEED, 2 ** 64 - 1, 1 << 63):
        coords = IS.Coords('device key', key, IS.ROW_OFFSET, 6)
        plain = p.call(coords)
        held = p.call(coords, seed=torch.tensor([key - 2 ** 64 if key >= 2 ** 63 else key], dtype=torch.int64, device=DEV))
        for call in (plain, held):
            assert_kernels(call, fwd=case.fwd)
            if test in LEAN_VARIANT:
                assert engine.lean_variant(call) == LEAN_VARIANT[test]
        assert held.desc.seed == 0 and held.desc.seed_dev and not plain.desc.seed_dev
        want = plain.launch().clone()
        assert torch.isfinite(want).all()
        assert torch.equal(held.launch(), want), (test, hex(key))
        outs.append(want)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


@pytest.mark.parametrize('test', ['lean specialised', 'generic srk'])
def test_the_criterion_sees_a_launch_one_row_or_one_step_off(test):
    """What step (c) resolves, on the GPU: against the oracle on the increments written at the base coordinates the inference launch
    passes, and the same launch one global row or one global step on misses the criterion's mean bound by two orders of magnitude -
    the figure tests/test_inference_stream_cpu.py asserts for the float32 oracle."""
    case = next(c for c in CASES if c.test == test)
    p = _problem(case)
    base = IS.Coords('base', IS.SEED, IS.ROW_OFFSET, 0)
    written = p.call(base, save_dW=True)
    written.launch()
    ref64, cpu32 = _reference(p, written.dW_out.cpu().numpy(), written.dU_out.cpu().numpy() if case.method == 'srk' else None)
    assert_parity(p.call(base).launch().cpu().numpy(), ref64, cpu32, what=test)
    for coords in (IS.Coords('next row', IS.SEED, IS.ROW_OFFSET + 1, 0), IS.Coords('next step', IS.SEED, IS.ROW_OFFSET, 1)):
        call = p.call(coords)
        assert_kernels(call, fwd=case.fwd)
        got = call.launch().cpu().numpy()
        rep = parity_report(got, ref64, cpu32)
        print(test, coords.name, rep)
        assert rep['mean'] >= 100 * 1e-5, (test, coords.name, rep)
        with pytest.raises(AssertionError):
            assert_parity(got, ref64, cpu32, what=f'{test}: {coords.name}')


def test_solve_call_refuses_rows_outside_32_bits():
    case = CASES[1]
    p = _problem(case)
    for bad in (-1, 2 ** 32 - case.B + 1, 2 ** 32):
        with pytest.raises(ValueError, match='row_offset'):
            p.call(IS.Coords('bad rows', IS.SEED, bad, 0))
        with pytest.raises(ValueError, match='row_offset'):
            p.call(IS.Coords('bad rows', IS.SEED, bad, 0), global_rows=2 ** 40)
