"""Training through model ensembles on the host (SNSDE_FLAG_ENSEMBLE_GRAD, options={'ensemble_grad': True}): the flag in the C ABI
and its host-only queries - what it opens, what stays refused and with which code, the per-member blocks of the two backward
workspaces - and sdeint_ensemble / Ensemble under autograd on CPU tensors against the loop of differentiable calls.
No GPU compute."""
import ctypes as C

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model, flip_batch, net_model
from tests.test_ensemble_cpu import _members, _wrappers

ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4, -5
P = C.c_void_p(4096)
EG = 256
PLANES = ('act_save', 'stage_save', 'traj', 'dW_out', 'dU_out')


def _solve(model, batch, members=0, kernel='auto', method=0, flags=0, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method, s.members = model, batch, KNOTS, STEPS, 2, method, members
    s.kernel, s.flags = _lib.KERNELS[kernel], flags
    if method == 2:
        s.srk_tab = P
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _train(s):
    """The descriptor with the planes a training forward of its method writes."""
    s.traj = s.act_save = s.dW_out = P
    if s.method == 2:
        s.stage_save = s.dU_out = P
    return s


def _path(s):
    return _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(s))]


def _layout(s):
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.lib().snsde_save_layout(C.byref(s), C.byref(a), C.byref(b), C.byref(c))
    return rc, a.value, b.value, c.value


def _backward(s):
    b = _lib.Backward()
    b.fwd = s
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(b.fwd, f, P)
    b.grad_ys = b.adj = b.workspace = b.delta_save = P
    return b


def test_abi_is_unchanged_and_the_flag_is_256():
    lib = _lib.lib()
    assert _lib.FLAG_ENSEMBLE_GRAD == EG
    assert C.sizeof(_lib.Solve) == 304 and lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0


@pytest.mark.parametrize('members', [0, 1])
def test_the_flag_has_no_effect_on_one_model(members):
    """The descriptor list of test_ensemble_cpu.test_zero_and_one_member_answer_as_before, with and without the flag."""
    lib = _lib.lib()
    wide = engine.model_struct(3, 48, 48, 2, 4, 17)
    cases = [(elementwise_model(64), 24, 'auto', 0), (elementwise_model(128), 24, 'mfma4', 1), (elementwise_model(128), 24, 'mfma4', 2),
             (net_model(), 24, 'auto', 0), (elementwise_model(256), 24, 'auto', 0), (wide, 24, 'auto', 0),
             (elementwise_model(128), 13, 'generic', 0), (elementwise_model(64), flip_batch(64), 'auto', 0)]
    for model, batch, kernel, method in cases:
        for train in (False, True):
            base, s = _solve(model, batch, members, kernel, method), _solve(model, batch, members, kernel, method, flags=EG)
            if train:
                _train(base), _train(s)
            assert _path(s) == _path(base) != 'none'
            assert engine.forward_kernel(s) == engine.forward_kernel(base)
            assert engine.backward_kernel(s) == engine.backward_kernel(base)
            assert lib.snsde_workspace_bytes(C.byref(s)) == lib.snsde_workspace_bytes(C.byref(base)) > 0
            assert lib.snsde_backward_supported(C.byref(s)) == lib.snsde_backward_supported(C.byref(base))
            assert _layout(s) == _layout(base)
            bs, bb = _backward(s), _backward(base)
            assert lib.snsde_backward_workspace_bytes(C.byref(bs)) == lib.snsde_backward_workspace_bytes(C.byref(bb))
            assert lib.snsde_param_gradients_workspace_bytes(C.byref(bs)) == lib.snsde_param_gradients_workspace_bytes(C.byref(bb))


@pytest.mark.parametrize('H', [64, 128])
def test_covered_ensembles_plan_the_general_adjoint(H):
    """members = 3, 24 rows: backward mode 1 on the general adjoint for auto and mfma4 under the three methods; the layout is the
    member-alone shard's and the two backward workspaces are 3 blocks of its own, each rounded up to 16 bytes (include/snsde.h)."""
    lib = _lib.lib()
    model = elementwise_model(H)
    for kernel in ('auto', 'mfma4'):
        for method, rev in ((0, 'general'), (1, 'general'), (2, 'general_srk')):
            s = _train(_solve(model, 24, 3, kernel, method, flags=EG))
            assert lib.snsde_backward_supported(C.byref(s)) == 1, (kernel, method)
            assert engine.backward_kernel(s) == rev
            assert _path(s) != 'none'
            assert engine.forward_kernel(s) == ('lean' if method != 2 else 'general_m4')
            # without the flag: the parent's answers
            off = _train(_solve(model, 24, 3, kernel, method))
            assert lib.snsde_backward_supported(C.byref(off)) == 0 and _path(off) == 'none' and engine.backward_kernel(off) == 'none'
            assert lib.snsde_backward_supported(C.byref(_solve(model, 24, 3, kernel, method))) == 0
            one = _train(_solve(model, 8, 0, kernel, method, row_offset=8, global_rows=24))
            assert engine.forward_kernel(one) == engine.forward_kernel(s) and engine.backward_kernel(one) == rev
            assert _layout(s) == _layout(one) and _layout(s)[0] == 0 and _layout(s)[3] > 0
            b, b1 = _backward(s), _backward(one)
            for query in (lib.snsde_backward_workspace_bytes, lib.snsde_param_gradients_workspace_bytes):
                alone = int(query(C.byref(b1)))
                assert alone > 0 and int(query(C.byref(b))) == 3 * ((alone + 15) & ~15), (query, alone)
            # the control-path gradient of an ensemble is not built: the front end sums the members' own
            assert lib.snsde_coeff_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED
            assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(b)) == 0
            assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(b1)) > 0
    q = engine.query_descriptor(model, 24, KNOTS, STEPS, 'euler', members=3, ensemble_grad=True, training=True)
    assert engine.backward_kernel(q) == 'general' and engine.forward_kernel(q) == 'lean'
    assert engine.forward_path(model, 24, KNOTS, STEPS, members=3, ensemble_grad=True, training=True) == 'lean'
    assert engine.forward_path(model, 24, KNOTS, STEPS, members=3, training=True) == 'none'
    grid = type('G', (), {'N': STEPS, 'T': 2})
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', members=3, ensemble_grad=True) == 1
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', members=3) == 0
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', ensemble_grad=True) == engine.backward_mode(model, 24, KNOTS, grid, 'euler') == 1


def test_what_stays_refused_with_the_flag():
    lib = _lib.lib()
    lean64 = elementwise_model(64)
    table = engine.model_struct(3, 64, 64, 2, 4, 13)
    sqrt_y = engine.model_struct(3, 64, 64, 2, 4, 7)
    net128 = engine.model_struct(3, 128, 128, 2, 1, 18)
    refused = [
        _solve(lean64, 24, 3, 'generic', flags=EG), _solve(lean64, 48, 3, 'mfma16', flags=EG), _solve(net_model(), 24, 3, flags=EG),
        _solve(net_model(), 24, 3, 'w4', flags=EG), _solve(net_model(), 24, 3, 'mfma4', flags=EG), _solve(net128, 24, 3, flags=EG),
        _solve(elementwise_model(256), 24, 3, flags=EG), _solve(lean64, 3 * flip_batch(64), 3, flags=EG),
        _solve(elementwise_model(128), 24, 3, flags=EG | _lib.FLAG_TWO_TILE),
        _solve(lean64, 24, 3, flags=EG, samples=2), _solve(lean64, 24, 3, flags=EG, z0_weight=P, z0_bias=P),
        _solve(table, 24, 3, flags=EG, noise_table=P), _solve(lean64, 24, 3, flags=EG, kl_column1=3),
        _solve(lean64, 24, 3, flags=EG | _lib.FLAG_BF16_OPERANDS), _solve(lean64, 24, 3, flags=EG | _lib.FLAG_BF16_OPERANDS | _lib.FLAG_BF16_GRAD),
        _solve(sqrt_y, 24, 3, method=1, flags=EG), _solve(engine.model_struct(3, 64, 64, 2, 4, 17, activation=1), 24, 3, flags=EG),
    ]
    for s in refused:
        _train(s)
        what = (s.kernel, s.flags, s.model.hidden_channels, s.model.noise_option, s.batch)
        assert lib.snsde_backward_supported(C.byref(s)) == 0, what
        assert engine.backward_kernel(s) == 'none', what
        assert _path(s) == 'none', what
        b = _backward(s)
        b.fwd.workspace_bytes = 1 << 30
        b.workspace_bytes = 1 << 30
        assert lib.snsde_solve_backward(C.byref(b), None) in (ERR_UNSUPPORTED, ERR_DIMS), what
        assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 30, None) in (ERR_UNSUPPORTED, ERR_DIMS), what
        assert lib.snsde_param_gradients(C.byref(b), P, P, 1 << 30, None) in (ERR_UNSUPPORTED, ERR_DIMS), what
        assert lib.snsde_param_gradients_workspace_bytes(C.byref(b)) == 0, what
        assert lib.snsde_solve_forward(C.byref(b.fwd), None) in (ERR_UNSUPPORTED, ERR_DIMS), what
    # the vector-field probe stays one model's
    s = _solve(lean64, 24, 3, flags=EG, params=P, coeffs=P, workspace=P)
    assert lib.snsde_eval_fg(C.byref(s), P, P, P, P, None) == ERR_UNSUPPORTED
    # a sqrt(y) diffusion under Euler is covered (the theta partials without a table); inference with the flag is the parent's
    assert lib.snsde_backward_supported(C.byref(_train(_solve(sqrt_y, 24, 3, flags=EG)))) == 1
    assert _path(_solve(lean64, 24, 3, flags=EG)) == _path(_solve(lean64, 24, 3)) == 'lean'


def test_backward_entry_points_validate_before_they_touch_memory():
    lib = _lib.lib()
    for method in (0, 1, 2):
        b = _backward(_train(_solve(elementwise_model(64), 24, 3, method=method, flags=EG)))
        b.workspace_bytes = 0
        assert lib.snsde_solve_backward(C.byref(b), None) == ERR_WORKSPACE
        assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_WORKSPACE
        assert lib.snsde_param_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_WORKSPACE
        b.workspace_bytes = int(lib.snsde_backward_workspace_bytes(C.byref(b)))
        assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 16, None) == ERR_WORKSPACE      # (the gradient pass's own workspace)
        assert lib.snsde_param_gradients(C.byref(b), P, P, 16, None) == ERR_WORKSPACE
        b.workspace_bytes -= 1
        assert lib.snsde_solve_backward(C.byref(b), None) == ERR_WORKSPACE
        b.fwd.flags = 0      # without the opt-in: refused as before
        assert lib.snsde_solve_backward(C.byref(b), None) == ERR_UNSUPPORTED


# ---- sdeint_ensemble / Ensemble under autograd on CPU tensors ------------------------------------------------------------------

def _grads(sdes):
    return [[None if p.grad is None else p.grad.clone() for p in sde.parameters()] for sde in sdes]


def _zero(sdes):
    for sde in sdes:
        for p in sde.parameters():
            p.grad = None


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_cpu_ensemble_grad_equals_the_loop_of_differentiable_solves(method):
    sdes, y0, times = _members()
    for sde in sdes:
        sde.requires_grad_(True)
    ts = torch.tensor([0., 1.3, 2.2, 5.])
    cot = torch.randn(4, 3, 4, 16, generator=torch.Generator().manual_seed(2))
    ya = y0.clone().requires_grad_(True)
    got = S.sdeint_ensemble(sdes, ya, ts, method=method, dt=0.5, options={'seed': 11, 'ensemble_grad': True})
    (got * cot).sum().backward()
    mine, _ = _grads(sdes), _zero(sdes)
    yb = y0.clone().requires_grad_(True)
    ref = torch.stack([S.sdeint(sde, yb[m], ts, method=method, dt=0.5, options={'seed': 11, 'row_offset': 4 * m, 'global_rows': 12})
                       for m, sde in enumerate(sdes)], dim=1)
    (ref * cot).sum().backward()
    assert torch.equal(got, ref) and torch.equal(ya.grad, yb.grad) and ya.grad.abs().max() > 0
    for gm, gr in zip(mine, _grads(sdes)):
        assert all(torch.equal(a, b) for a, b in zip(gm, gr)) and any(a.abs().max() > 0 for a in gm)
    with pytest.raises(NotImplementedError, match='strict'):
        S.sdeint_ensemble(sdes, ya, ts, method=method, dt=0.5, options={'seed': 11, 'ensemble_grad': True, 'strict': True})
    with pytest.raises(ValueError, match='inference only'):      # no opt-in: the parent's refusal, word for word
        S.sdeint_ensemble(sdes, ya, ts, method=method, dt=0.5, options={'seed': 11})


def test_cpu_coefficient_gradient_is_the_sum_over_the_members():
    sdes, y0, times = _members()
    ts = torch.tensor([0., 2.2, 5.])
    base = sdes[0].coeffs.clone()
    total = None
    for m, sde in enumerate(sdes):
        c = base.clone().requires_grad_(True)
        sde.set_X(c, times)
        S.sdeint(sde, y0[m], ts, method='euler', dt=0.5, options={'seed': 5, 'row_offset': 4 * m, 'global_rows': 12}).sum().backward()
        total = c.grad if total is None else total + c.grad
    c = base.clone().requires_grad_(True)
    for sde in sdes:
        sde.set_X(c, times)
    S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'seed': 5, 'ensemble_grad': True}).sum().backward()
    assert c.grad.abs().max() > 0 and torch.allclose(c.grad, total, rtol=1e-5, atol=1e-6)      # (autograd's own order of the M sums)
    # the same graph built by hand gives the same bits
    c2 = base.clone().requires_grad_(True)
    for sde in sdes:
        sde.set_X(c2, times)
    torch.stack([S.sdeint(sde, y0[m], ts, method='euler', dt=0.5, options={'seed': 5, 'row_offset': 4 * m, 'global_rows': 12})
                 for m, sde in enumerate(sdes)], dim=1).sum().backward()
    assert torch.equal(c.grad, c2.grad)


def test_option_conflicts_and_the_strict_bool():
    sdes, y0, times = _members()
    ts = torch.tensor([0., 2.2, 5.])
    ya = y0.clone().requires_grad_(True)
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='ensemble_grad must be a bool'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_grad': bad})
        with pytest.raises(ValueError, match='ensemble_grad must be a bool'):
            engine.check_ensemble_grad(bad)
    assert engine.check_ensemble_grad(True) is True and engine.check_ensemble_grad(False) is False
    conflicts = ({'samples': 2}, {'save_traj': True}, {'recompute': 2}, {'z0_linear': torch.nn.Linear(3, 16)}, {'sample_grad': True},
                 {'bf16_grad': True}, {'precision': 'bf16'}, {'param_pass': 'torch'})
    for opt in conflicts:
        with pytest.raises(ValueError):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=0.5, options=dict(opt, ensemble_grad=True))


def test_recompute_in_the_environment_is_a_conflict(monkeypatch):
    sdes, y0, times = _members()
    monkeypatch.setenv('SNSDE_RECOMPUTE_STEPS', '2')
    with pytest.raises(ValueError, match='recompute'):
        S.sdeint_ensemble(sdes, y0.clone().requires_grad_(True), torch.tensor([0., 2.2, 5.]), method='euler', dt=0.5,
                          options={'ensemble_grad': True})


def test_solvecall_without_the_opt_in_raises_as_before():
    # (SolveCall checks its arguments before it touches the device: CPU tensors get as far as the members check)
    model = elementwise_model(64)
    y0 = torch.zeros(24, 64)
    with pytest.raises(ValueError, match='inference only'):
        engine.SolveCall(model, torch.zeros(3, 8), torch.zeros(8, KNOTS - 1, 12), None, y0, members=3, save_traj=True)


@pytest.mark.parametrize('kind', [S.NeuralSDE, S.IstsNeuralSDE])
def test_cpu_ensemble_module_trains_like_the_wrappers(kind):
    models, coeffs, times = _wrappers(kind)
    M, B = len(models), coeffs.shape[0]
    for net in models:
        net.train().requires_grad_(True)
    ens = S.Ensemble(models).train()
    fi = torch.tensor([5, 3, 5, 2])
    args = (coeffs, times) if kind is S.IstsNeuralSDE else (times, (coeffs,), fi)
    first = (lambda o: o[0]) if kind is S.IstsNeuralSDE else (lambda o: o)
    torch.manual_seed(123)      # (the classification head's Dropout draws per member, in member order in both arms)
    got = first(ens(*args, options={'seed': 7, 'ensemble_grad': True}))
    cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(1))
    (got * cot).sum().backward()
    mine = [[p.grad.clone() for p in net.parameters()] for net in models]
    for net in models:
        net.zero_grad(set_to_none=True)
    torch.manual_seed(123)
    refs = torch.stack([first(net(*args, options={'seed': 7, 'row_offset': m * B, 'global_rows': M * B})) for m, net in enumerate(models)])
    (refs * cot).sum().backward()
    assert torch.equal(got, refs)
    for gm, net in zip(mine, models):
        assert all(torch.equal(a, p.grad) for a, p in zip(gm, net.parameters()))
        assert any(a.abs().max() > 0 for a in gm)
    with pytest.raises(ValueError, match='inference only'):
        ens(*args, options={'seed': 7})
