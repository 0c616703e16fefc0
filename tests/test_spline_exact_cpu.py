"""Spline coefficient construction against exact-rational known answers, on the host.

tests/golden/spline_exact.npz holds, for float32-representable inputs, the coefficients of both constructions
(`natural_cubic_spline_coeffs`, `hermite_cubic_coefficients_with_backward_differences`) computed with fractions.Fraction from
their definitions by tests/golden/make_spline_exact_golden.py, which imports nothing from oracle/ or the package and asserts
every definition before it writes.  Against them, here:

  * the generator reproduces the committed fixture;
  * the numpy oracle in float64 (the arbiter of most GPU parity tests): 1e-12 of max(1, max |component|);
  * the package's tensor-op constructions on CPU float32 tensors: the float32 bound of tests/spline_exact_cases.py (4 x the
    float32 oracle's own error, per kind and component), exact zeros where exact arithmetic AND any correct float32 construction
    give 0, and the float32 image of the rational bit for bit on the series where no float32 operation rounds.

The exact-zero assertion is what a natural spline through two knots needs: the reference (interpolate.py:16-20), the oracle and
the HIP kernel take a linear branch there; a Thomas solve of the 2 x 2 system returns curvature of round-off size instead
(before `controldiffeq._series_coeffs` had that branch: `two_c` = -7.05e-6, `three_d` = 5.22e-5 on the fixture's `short2`
series without NaN, t = [0, 0.2704]; profiles/spline_exact_margins.txt)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from tests import spline_exact_cases as E
from tests.helpers import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location('make_spline_exact_golden', os.path.join(GOLDEN, 'make_spline_exact_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_the_committed_fixture(tmp_path):
    path = _generator().main(str(tmp_path))
    new = np.load(path, allow_pickle=False)
    assert sorted(new.files) == sorted(E.EX.files)
    for k in new.files:
        a, b = new[k], E.EX[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == 'f':
            np.testing.assert_array_equal(a.view(f'u{a.dtype.itemsize}'), b.view(f'u{b.dtype.itemsize}'), err_msg=k)
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)
    with open(path, 'rb') as f, open(os.path.join(GOLDEN, E.FIXTURE), 'rb') as g:
        assert f.read() == g.read()


def test_fixture_holds_what_the_tests_rely_on():
    assert E.CASES == ['dyadic_unit', 'dyadic_pow2', 'irregular', 'edges', 'short2', 'short3']
    two_knot = 0
    for tag in E.CASES:
        c = E.case(tag)
        S_, L = c['X'].shape
        assert c['times'].dtype == np.float32 and c['X'].dtype == np.float32 and 2 <= L <= 12
        for kind in E.KINDS:
            assert c[kind].dtype == np.float64 and c[kind].shape == (S_, L - 1, 4) and c['zero_' + kind].shape == (S_, L - 1, 4)
            assert (c[kind][c['zero_' + kind]] == 0).all()
        knots = (~np.isnan(c['X'])).copy()
        knots[:, 0] = knots[:, -1] = True
        two_knot += int(((knots.sum(1) == 2) & (~np.isnan(c['X'])).any(1)).sum())
        assert c['hermite_bit_exact'].all() == tag.startswith('dyadic') and c['hermite_bit_exact'].any() == tag.startswith('dyadic')
    assert two_knot >= 8


@pytest.mark.parametrize('tag', E.CASES)
@pytest.mark.parametrize('kind', E.KINDS)
def test_float64_oracle_against_the_exact_values(kind, tag):
    got = E.oracle(kind, tag, np.float64)
    want = E.case(tag)[kind]
    err = np.abs(got - want).max(axis=(0, 1))
    tol = 1e-12 * np.maximum(1.0, np.abs(want).max(axis=(0, 1)))
    print(f'{kind} {tag}: float64 oracle |err| per component {err}, allowed {tol}')
    assert (err <= tol).all(), (err, tol)


@pytest.mark.parametrize('kind', E.KINDS)
def test_float32_oracle_gives_the_exact_zeros_and_the_bit_exact_series(kind):
    """The yardstick satisfies what is asked of the implementations (its ratio to e32 is at most 1 by construction)."""
    for tag in E.CASES:
        r = E.check(kind, tag, E.oracle(kind, tag, np.float32), 'oracle32')
        assert (r <= 1.0).all()


@pytest.mark.parametrize('tag', E.CASES)
@pytest.mark.parametrize('kind', E.KINDS)
def test_host_tensor_ops_float32_within_the_bound_exact_zeros_bit_exact_series(kind, tag):
    E.check(kind, tag, E.host_coeffs(kind, tag), 'host cpu')


@pytest.mark.parametrize('tag', E.CASES)
@pytest.mark.parametrize('kind', E.KINDS)
def test_host_tensor_ops_float64_against_the_exact_values(kind, tag):
    got = E.host_coeffs(kind, tag, torch.float64)
    want = E.case(tag)[kind]
    err = np.abs(got - want).max(axis=(0, 1))
    assert (err <= 1e-12 * np.maximum(1.0, np.abs(want).max(axis=(0, 1)))).all(), err
    assert (got[E.case(tag)['zero_' + kind]] == 0.0).all()


def test_two_knot_natural_series_are_straight_lines_with_exact_zero_curvature():
    """The defect this file was written for, on its own: every series of the fixture whose knots compact to two."""
    n = 0
    for tag in E.CASES:
        c = E.case(tag)
        obs = ~np.isnan(c['X'])
        knots = obs.copy()
        knots[:, 0] = knots[:, -1] = True
        rows = np.flatnonzero((knots.sum(1) == 2) & obs.any(1))
        if rows.size == 0:
            continue
        got = E.host_coeffs('natural', tag)[rows]
        print(f'{tag}: two-knot series {[str(s) for s in c["names"][rows]]}: max |two_c| {np.abs(got[..., 2]).max():.3e}, '
              f'max |three_d| {np.abs(got[..., 3]).max():.3e}')
        assert (got[..., 2] == 0.0).all() and (got[..., 3] == 0.0).all(), (tag, got[..., 2:])
        # one subtraction, one division: b is the float32 quotient of the float32 difference, on every interval
        t = c['times']
        for r, g in zip(rows, got):
            x = c['X'][r]
            x0 = x[obs[r]][0] if not obs[r, 0] else x[0]
            x1 = x[obs[r]][-1] if not obs[r, -1] else x[-1]
            slope = np.float32(np.float32(x1 - x0) / np.float32(t[-1] - t[0]))
            assert (g[:, 1] == slope).all(), (tag, r)
        n += rows.size
    assert n >= 8


def test_gradient_through_the_two_knot_branch_is_finite_and_that_of_the_line():
    """SNSDE_SPLINE_GRAD=torch differentiates this statement: the branch torch.where discards must not leak NaN or inf."""
    t = torch.tensor([0.0, 0.2704, 0.9, 1.7], dtype=torch.float64)
    X = torch.tensor([[-2.012, float('nan'), float('nan'), 1.104],        # ends only
                      [float('nan'), 0.3, float('nan'), float('nan')],     # one observation
                      [0.5, -0.25, 1.5, 0.75]], dtype=torch.float64).T[None].clone().requires_grad_(True)
    a, b, c2, d3 = S.controldiffeq.natural_cubic_spline_coeffs(t, X)
    g = torch.autograd.grad(b[0, :, 0].sum() + (c2 ** 2).sum() + (d3 ** 2).sum() + a[0, :, 1].sum(), X)[0]
    assert bool(torch.isfinite(g[~torch.isnan(X.detach())]).all()) and bool((g[torch.isnan(X.detach())] == 0).all())
    h = float(t[3] - t[0])
    # series 0 contributes only through b (its two_c, three_d are constants 0): d b / d x = -+ 1 / h on each of 3 intervals
    np.testing.assert_allclose(g[0, [0, 3], 0].numpy(), [-3 / h, 3 / h], rtol=1e-14)
    np.testing.assert_allclose(float(g[0, 1, 1]), 3.0, rtol=1e-14)          # a = the one observation on all 3 intervals
