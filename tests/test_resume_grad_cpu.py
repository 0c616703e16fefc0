"""Training through continued solves on the host (SNSDE_FLAG_RESUME_GRAD, options={'resume_grad': True}): the flag and the _at
backward entry points in the header, the binding and the library; their validation codes; the front end's refusals with and
without the opt-in; and, on the tensor-op loop with a Brownian stub that carries its path, a cut differentiable solve whose
gradients equal the uncut one's (float64, autograd both ways).  No GPU compute."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model
from tests.test_step_offset_cpu import TS, Stub, _launch_rc, _model, _solve

ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED = -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(4096)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------

def test_the_flag_and_the_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'snsde.h')).read()
    assert re.search(r'SNSDE_FLAG_RESUME_GRAD\s*=\s*4096', header) and _lib.RESUME_GRAD == 4096
    assert re.search(r'^SNSDE_API\s+int\s+snsde_solve_backward_at\(const snsde_backward\* b, int64_t step_offset, void\* hip_stream\);', header, re.M)
    assert re.search(r'^SNSDE_API\s+int\s+snsde_backward_with_gradients_at\(', header, re.M)
    L = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ('snsde_solve_backward_at', 'snsde_backward_with_gradients_at'):
        assert name in _lib.EXPORTS and re.search(rf'\bT {name}$', dyn, re.M)
    assert L.snsde_solve_backward_at.argtypes == [C.POINTER(_lib.Backward), C.c_int64, C.c_void_p]
    assert L.snsde_backward_with_gradients_at.argtypes == [C.POINTER(_lib.Backward), C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p]
    # the offset is a launch argument: no struct and no version moved, and no plan reads the flag (it is not in the configuration record)
    assert C.sizeof(_lib.Solve) == 304 and L.snsde_version() == 2
    assert 'resume_grad' not in engine.SolveConfig._fields
    assert inspect.signature(engine.SolveCall.__init__).parameters['resume_grad'].default is False
    assert engine.check_resume_grad(True) is True
    with pytest.raises(ValueError, match=r'^resume_grad must be a bool \(.*\), got 1$'):
        engine.check_resume_grad(1)


def test_the_forward_accepts_training_planes_at_an_offset_under_the_flag_only():
    model = elementwise_model(32)
    train = dict(act_save=P, traj=P)
    accepted = _launch_rc(_solve(model, **train))      # (the code behind every check of the offset: the missing workspace)
    assert accepted not in (0, ERR_DIMS, ERR_UNSUPPORTED)
    assert _launch_rc(_solve(model, **train), 5) == ERR_UNSUPPORTED
    assert _launch_rc(_solve(model, flags=_lib.RESUME_GRAD, **train), 5) == accepted
    assert _launch_rc(_solve(model, flags=_lib.RESUME_GRAD, **train), 0) == accepted
    srk = dict(method=2, srk_tab=P, stage_save=P, act_save=P, traj=P, dW_out=P, dU_out=P)
    assert _launch_rc(_solve(model, **srk), 5) == ERR_UNSUPPORTED
    assert _launch_rc(_solve(model, flags=_lib.RESUME_GRAD, **srk), 5) == _launch_rc(_solve(model, **srk))
    # z0_weight stays refused, and the range check stays in front
    assert _launch_rc(_solve(model, flags=_lib.RESUME_GRAD, z0_weight=P, z0_bias=P), 5) == ERR_UNSUPPORTED
    assert _launch_rc(_solve(model, flags=_lib.RESUME_GRAD, **train), -1) == ERR_DIMS
    assert _launch_rc(_solve(model, flags=_lib.RESUME_GRAD, **train), 2 ** 31 - STEPS) == ERR_DIMS


def _backward(model, flags=0, **kw):
    b = _lib.Backward()
    b.struct_size = C.sizeof(_lib.Backward)
    s = _solve(model, flags=flags, act_save=P, traj=P, **kw)
    s.struct_size = C.sizeof(_lib.Solve)
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(s, f, P)
    b.fwd = s
    b.grad_ys = b.adj = b.workspace = b.delta_save = P
    b.workspace_bytes = 0
    return b


def test_the_backward_calls_check_the_offset_before_any_launch():
    model = elementwise_model(32)
    L = _lib.lib()
    solve = lambda b, n0: L.snsde_solve_backward_at(C.byref(b), n0, None)
    both = lambda b, n0: L.snsde_backward_with_gradients_at(C.byref(b), P, P, 0, n0, None)
    for call, old in ((solve, lambda b: L.snsde_solve_backward(C.byref(b), None)),
                      (both, lambda b: L.snsde_backward_with_gradients(C.byref(b), P, P, 0, None))):
        accepted = old(_backward(model))      # (a valid descriptor without a workspace)
        assert accepted not in (0, ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED)
        assert call(_backward(model), 0) == accepted and call(_backward(model, _lib.RESUME_GRAD), 0) == accepted
        assert call(_backward(model), 5) == ERR_UNSUPPORTED
        assert call(_backward(model, _lib.RESUME_GRAD), 5) == accepted
        assert call(_backward(model, _lib.RESUME_GRAD), 2 ** 31 - 1 - STEPS) == accepted
        for bad in (-1, 2 ** 31 - STEPS, 2 ** 40):
            assert call(_backward(model, _lib.RESUME_GRAD), bad) == ERR_DIMS and call(_backward(model), bad) == ERR_DIMS
    assert L.snsde_solve_backward_at(None, 0, None) == ERR_NULL and L.snsde_backward_with_gradients_at(None, P, P, 0, 0, None) == ERR_NULL


# ---- the front end ----------------------------------------------------------------------------------------------------------

def test_refusals_with_and_without_the_opt_in(monkeypatch):
    m, pr = _model()
    y0 = torch.from_numpy(pr['y0'])
    m.requires_grad_(True)
    state = (torch.tensor([3, 0, 0]),)
    # without the opt-in (and with it switched off) every refusal is the old one
    for options in ({'step_offset': 3}, {'step_offset': 3, 'resume_grad': False}):
        with pytest.raises(ValueError, match='step_offset=3 is inference only.*a continued solve has no backward'):
            S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', options=options)
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', extra_solver_state=state)
    with pytest.raises(ValueError, match='resume_grad must be a bool'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', options={'resume_grad': 1})
    # with it: recompute, the environment's recompute, z0_linear on a continued piece - each named
    on = {'step_offset': 3, 'resume_grad': True}
    with pytest.raises(ValueError, match='resume_grad=True .* does not take recompute'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', options=dict(on, recompute=2))
    monkeypatch.setenv('SNSDE_RECOMPUTE_STEPS', '2')
    with pytest.raises(ValueError, match='resume_grad=True .* does not take recompute'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', options=dict(on))
    monkeypatch.delenv('SNSDE_RECOMPUTE_STEPS')
    with pytest.raises(ValueError, match='resume_grad=True .* does not take z0_linear on a continued piece'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', options=dict(on, z0_linear=torch.nn.Linear(3, 16)))
    # the first piece may still start from the initial network
    ys = S.sdeint(m, y0, TS[:2], bm=Stub(), dt=0.25, method='euler', options={'resume_grad': True, 'z0_linear': torch.nn.Linear(3, 16)})
    assert ys.requires_grad
    # an ensemble keeps its own text, whatever the option says
    with pytest.raises(ValueError, match='step_offset=3 is inference only'):
        S.sdeint_ensemble([m, m], y0[None].repeat(2, 1, 1), TS, bm=Stub(), dt=0.25, method='euler',
                          options={'step_offset': 3, 'ensemble_grad': True, 'resume_grad': True})
    # a route that would draw from a torch generator cannot continue a path, differentiated or not
    for options in (on, dict(on, backend='torch'), dict(on, samples=2, sample_grad=True)):
        with pytest.raises(NotImplementedError, match='fused solve.*caller-supplied `bm`'):
            S.sdeint(m, y0, TS, dt=0.25, method='euler', options=options)


@pytest.mark.parametrize('method', ['euler', 'milstein', 'srk'])
def test_a_cut_differentiable_solve_has_the_gradients_of_the_uncut_one(method):
    """float64, the tensor-op loop, a `bm` that carries its path: the states are equal bit for bit, and every gradient up to the order of
    the one sum autograd forms over the pieces."""
    m, pr = _model()
    m = m.double().requires_grad_(True)
    m.set_X(torch.from_numpy(pr['coeffs']).double().requires_grad_(True), torch.from_numpy(pr['times']).double())
    y0 = torch.from_numpy(pr['y0']).double().requires_grad_(True)
    ts = TS.double()
    leaves = [y0, m.coeffs] + list(m.parameters())
    weight = torch.randn(4, 4, 16, generator=torch.Generator().manual_seed(1), dtype=torch.float64)

    class Stub64(Stub):
        def __call__(self, *a, **k):
            out = super().__call__(*a, **k)
            return tuple(o.double() for o in out) if isinstance(out, tuple) else out.double()

    whole = S.sdeint(m, y0, ts, bm=Stub64(), dt=0.25, method=method)
    want = torch.autograd.grad((whole * weight).sum(), leaves, allow_unused=True)
    for cuts in ((0, 1, 2, 3), (0, 2, 3)):
        y, state, pieces = y0, None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ys, state = S.sdeint(m, y, ts[a:b + 1], bm=Stub64(), dt=0.25, method=method, options={'resume_grad': True}, extra=True,
                                 extra_solver_state=state)
            pieces.append(ys if a == 0 else ys[1:])
            y = ys[-1]
        chained = torch.cat(pieces)
        assert torch.equal(chained, whole)
        got = torch.autograd.grad((chained * weight).sum(), leaves, allow_unused=True)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert torch.allclose(g, w, rtol=1e-12, atol=1e-13 * float(w.abs().max())), float((g - w).abs().max())
    # the low-level knob on a differentiated call, and truncated back-propagation: a detached hand-over cuts dL/dy0 only
    ys = S.sdeint(m, whole[1].detach(), ts[1:], bm=Stub64(), dt=0.25, method=method, options={'step_offset': 3, 'resume_grad': True})
    assert torch.equal(ys, whole[1:]) and ys.requires_grad


def test_the_filter_is_differentiable_on_cpu_tensors():
    m, pr = _model()
    m.requires_grad_(True)
    y0 = torch.from_numpy(pr['y0'])

    class Paths(Stub):      # (B S rows)
        def __init__(self):
            super().__init__((8, 16))

    obs = lambda k, yk: -0.5 * ((yk[:, :3].reshape(4, 2, 3) - 0.1 * k) ** 2).sum(-1) / 0.25
    for threshold in (0.0, 1.0):
        gen = lambda: torch.Generator().manual_seed(3)
        plain = S.sdeint_filter(m, y0, TS, obs, bm=Paths(), method='euler', dt=0.25, options={'samples': 2}, threshold=threshold, generator=gen())
        assert not plain.logz.requires_grad
        r = S.sdeint_filter(m, y0, TS, obs, bm=Paths(), method='euler', dt=0.25, options={'samples': 2}, threshold=threshold, generator=gen(),
                            differentiable=True)
        for a, b in zip(r, plain):
            assert torch.equal(a.detach(), b)
        assert r.logz.requires_grad and r.log_weight.requires_grad and r.ys.requires_grad
        assert not r.ancestor.requires_grad and not r.ess.requires_grad
        (-r.logz[-1].mean()).backward()
        grads = [p.grad for p in m.parameters()]
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
        m.zero_grad()
