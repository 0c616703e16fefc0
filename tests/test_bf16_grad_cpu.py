"""Training through the bf16-operand solve (options={'precision': 'bf16', 'bf16_grad': True}, SNSDE_FLAG_BF16_GRAD), the part that
needs no GPU: the straight-through reference against the numpy restatement, the host-side route queries, the option's refusals,
and the float32 yardstick of every case the GPU test compares (tests/bf16_grad_cases.py)."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests import bf16_grad_cases as K
from tests import bf16_grad_reference as R
from tests.bf16_reference import solve_bf16
from tests.golden.make_route_golden import FIELDS, answers
from tests.helpers import draw_dW, load, make_problem


@pytest.mark.parametrize('case', [(4, 17, 2, 6, 64, 5, 6, 'euler'), (2, 3, 1, 5, 64, 4, 5, 'milstein'), (0, 9, 3, 7, 128, 6, 6, 'milstein')],
                         ids=K.case_id)
def test_reference_forward_is_the_numpy_restatement(case):
    io, no, NL, B, H, C, L, method = case
    pr = make_problem(11, io, no, NL, B, H, C, L)
    ts = pr['times']
    dW = draw_dW(3, ts, 1.0, B, H)
    want, _ = solve_bf16(pr['params'], io, no, pr['coeffs'], pr['times'], pr['y0'], ts, 1.0, dW, method=method)
    with torch.no_grad():
        got = R.solve(R.Bf16GradField(pr), torch.from_numpy(pr['y0']).double(), ts, 1.0, torch.from_numpy(dW).double(), method)
    assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-12), np.abs(got.numpy() - want).max()
    # ... and the same field under the package's own tensor-op loop
    bm = iter(torch.from_numpy(dW).double())
    with torch.no_grad():
        loop = S.sdeint(R.Bf16GradField(pr), torch.from_numpy(pr['y0']).double(), torch.from_numpy(ts), bm=lambda a, b: next(bm), dt=1.0,
                        method=method, options={'backend': 'torch'})
    assert np.allclose(loop.numpy(), want, rtol=1e-12, atol=1e-12)


def test_straight_through_gradient_of_one_layer():
    """z = q(W) q(x) + b: dL/dx = q(W)^T delta, dL/dW = delta (x) q(x), dL/db = sum delta"""
    g = torch.Generator().manual_seed(0)
    W, x, b = (torch.randn(s, generator=g, dtype=torch.float64, requires_grad=True) for s in ((5, 7), (3, 7), (5,)))
    d = torch.randn(3, 5, generator=g, dtype=torch.float64)
    ((R.q(x) @ R.q(W).T + b) * d).sum().backward()
    qW, qx = R.round_bf16(W.detach().float()).double(), R.round_bf16(x.detach().float()).double()
    assert not torch.equal(qW, W.detach())
    assert torch.allclose(x.grad, d @ qW, rtol=1e-14) and torch.allclose(W.grad, d.T @ qx, rtol=1e-14) and torch.allclose(b.grad, d.sum(0))


def _k2(H=128, NL=2, io=4, no=17, C=21):
    return engine.model_struct(C, H, H, NL, io, no)


def _mode(model, method='euler', B=1024, L=101, **kw):
    times = np.arange(L, dtype=np.float32)
    grid = engine.StepGrid(np.array([0.0, L - 1.0], np.float32), 1.0, times, None)
    return engine.backward_mode(model, B, L, grid, method, **kw)


def test_backward_mode_under_the_flag():
    on = dict(precision='bf16', bf16_grad=True)
    assert _lib.FLAG_BF16_GRAD == 128 and engine.precision_flags('bf16', True) == 16 + 128 and engine.precision_flags('fp32', True) == 0
    assert _mode(_k2(), **on) == 1
    assert _mode(_k2(H=64, NL=3, io=1, no=3, C=5), 'milstein', B=37, L=9, **on) == 1
    assert _mode(_k2(), B=16384, **on) == 1          # (bf16 plans 4-row tiles at every batch size; so does its adjoint)
    # no plan: SRK, other hidden sizes, a diffusion net, sample paths, a supplied table, explicit generic / 16-row kernels - and no flag
    assert _mode(_k2(), 'srk', **on) == 0
    assert _mode(_k2(H=256), **on) == 0 and _mode(_k2(H=32), **on) == 0
    assert _mode(_k2(no=18), **on) == 0
    assert _mode(_k2(), samples=2, **on) == 0 and _mode(_k2(), samples=2, sample_grad=True, **on) == 0
    assert _mode(_k2(no=13), table=True, **on) == 0
    assert _mode(_k2(), kl_column=3, **on) == 0
    assert _mode(_k2(), kernel='generic', **on) == 0 and _mode(_k2(), kernel='mfma16', **on) == 0
    assert _mode(_k2(), precision='bf16') == 0
    # the flag alone means nothing: the fp32 answers
    assert _mode(_k2()) == 1 and _mode(_k2(), 'srk') == 1 and _mode(_k2(), precision='fp32', bf16_grad=True) == 1


def test_forward_path_with_training_planes():
    """the bf16 kernel takes the training planes under the flag only, and never hands them to another kernel"""
    assert engine.forward_path(_k2(), 1024, 101, 100, precision='bf16', training=True) == 'none'
    assert engine.forward_path(_k2(), 1024, 101, 100, precision='bf16', training=True, bf16_grad=True) == 'lean-bf16'
    assert engine.forward_path(_k2(), 1024, 101, 100, precision='bf16', bf16_grad=True) == 'lean-bf16'
    assert engine.forward_path(_k2(H=256), 1024, 101, 100, precision='bf16', training=True, bf16_grad=True) == 'none'
    assert engine.forward_path(_k2(), 1024, 101, 100, 'srk', precision='bf16', training=True, bf16_grad=True) == 'none'
    assert engine.forward_path(_k2(), 1024, 101, 100, precision='bf16', training=True, bf16_grad=True, samples=2) == 'none'
    assert engine.forward_path(_k2(no=13), 1024, 101, 100, table=True, precision='bf16', training=True, bf16_grad=True) == 'none'
    assert engine.forward_path(_k2(), 1024, 101, 100, training=True, bf16_grad=True) == 'lean'


def test_answers_without_the_flag_are_the_recorded_ones():
    g = load('routes.npz')
    desc, want = g['desc'], g['answers']
    fl, kn = FIELDS.index('flags'), FIELDS.index('kernel')
    asked = 0
    for row, exp in list(zip(desc, want))[::53]:
        if int(row[fl]) & _lib.FLAG_BF16_GRAD or int(row[kn]) in (3, 4, 5):     # (explicit tile kernels: test_routes_cpu's known changes)
            continue
        assert [int(v) for v in answers(row)] == [int(v) for v in exp], dict(zip(FIELDS, row))
        asked += 1
    assert asked >= 40


def _field(io=4, no=17, C=5, H=64, B=8, L=6):
    m = S.Diffusion_model(C, H, H, 2, input_option=io, noise_option=no)
    times = torch.arange(L, dtype=torch.float32)
    m.set_X(torch.zeros(B, L - 1, 4 * C), times)
    return m, torch.zeros(B, H), times


def test_option_errors_launch_nothing(monkeypatch):
    launched = []
    monkeypatch.setattr(engine.SolveCall, 'launch', lambda self, *a, **k: launched.append(1))
    m, y0, ts = _field()
    on = {'precision': 'bf16', 'bf16_grad': True}

    def refused(match, y=y0, **extra):
        with pytest.raises(ValueError, match=match):
            S.sdeint(m, y, ts, dt=1.0, method='euler', options=dict(on, **extra))

    with pytest.raises(ValueError, match='bool'):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'bf16', 'bf16_grad': 1})
    with pytest.raises(ValueError, match="precision='bf16'"):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'bf16_grad': True})
    with pytest.raises(ValueError, match="precision='bf16'"):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'fp32', 'bf16_grad': True})
    with pytest.raises(ValueError, match='inference'):        # without the opt-in: as before
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'bf16'})
    refused('CPU')
    refused('torch', backend='torch')
    refused('samples', samples=2)
    refused('samples', samples=2, sample_grad=True)
    refused('recompute', recompute=2)
    refused('param_pass', param_pass='torch')
    monkeypatch.setenv('SNSDE_RECOMPUTE_STEPS', '4')
    refused('SNSDE_RECOMPUTE_STEPS')
    monkeypatch.delenv('SNSDE_RECOMPUTE_STEPS')
    m.coeffs.requires_grad_(True)
    refused('control path')
    assert not launched


def test_selected_cases_span_the_covered_options():
    sel = K.selected()
    assert K.K2_CASES[0] in sel and K.K2_CASES[1] in sel
    assert {c[4] for c in sel} == {64, 128} and {c[2] for c in sel} == {1, 2, 3} and {c[7] for c in sel} == {'euler', 'milstein'}
    ios, nos = {c[0] for c in sel}, {c[1] for c in sel}
    assert 0 in ios and ios & {1, 3, 5} and ios & {2, 4, 6} and nos & {16, 17}
    assert len(sel) >= 12


@pytest.mark.parametrize('case', K.selected(), ids=K.case_id)
def test_float32_yardstick_stays_inside_the_bound(case):
    """Before any GPU run: the float32 reference ALONE, in the kernel's place, is inside the kink cap and, with its kink rows out of
    the loss, inside 1e-4 relative L2 per tensor - so max(4 e32, 1e-4) bounds the kernel by what float32 arithmetic does to THIS
    case's gradients.  Asked of the plain float32 run, of a second one with other roundings, and (the cap) of four runs from a y0
    jittered by one ulp: a case that only one lucky float32 run differentiates is no case (it is re-seeded: bf16_grad_cases.RESEED)."""
    _, g64, g32 = K.reference(case)
    for what, g in (('float32', g32), ('second float32 run', K.second_float32_run(case))):
        rows = K.kink_rows(g['y0'], g64['y0'])
        assert len(rows) <= K.kink_cap(case[3]), (what, rows)
        r64 = g64
        if rows:
            _, r64, g = K.reference(case, rows) if what == 'float32' else (None, K.reference(case, rows)[1], K.second_float32_run(case, rows))
        worst = {n: K.rel_l2(g[n], r64[n]) for n in r64 if float(r64[n].abs().max()) > 0}
        print(K.case_id(case), what, 'kink rows', rows, 'worst', max(worst.items(), key=lambda kv: kv[1]))
        assert all(v <= 1e-4 for v in worst.values()), (what, {n: v for n, v in worst.items() if v > 1e-4})
    for g in K.jittered_float32_runs(case):
        assert len(K.kink_rows(g, g64['y0'])) <= K.kink_cap(case[3])


def test_prepare_fold_is_the_float32_product():
    """the restated fold against float64: float32 round-off of a 128-term sum, and exactly the fmaf chains on a case small enough to
    write out"""
    rng = np.random.default_rng(0)
    E, W = rng.standard_normal((8, 128)).astype(np.float32), rng.standard_normal((128, 9)).astype(np.float32)
    F = R.prepare_fold(E, W)
    assert F.dtype == np.float32 and np.abs(F - E.astype(np.float64) @ W.astype(np.float64)).max() <= 128 * 2.0 ** -24 * np.abs(E).max() * np.abs(W).max() * 4
    E, W = np.array([[1.0, 2.0 ** -24, 3.0, -1.0, 2.0 ** -24]], np.float32), np.ones((5, 1), np.float32)
    # chains: a0 = fmaf(2^-24, 1, 1) = 1 (tie to even), a1 = 2^-24, a2 = 3, a3 = -1  ->  (1 + 2^-24) + 2 = 3 in float32
    assert R.prepare_fold(E, W)[0, 0] == np.float32(3.0)
