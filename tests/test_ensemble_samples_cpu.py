"""Sample paths of a model ensemble on the host (SNSDE_FLAG_ENSEMBLE_SAMPLES, options={'samples': S, 'ensemble_samples': True}):
the flag in the C ABI and its host-only queries - what it opens, what it leaves alone, the dimension errors, the three flags that
training needs - the two statistics exports, and sdeint_ensemble / Ensemble / ensemble_stats on CPU tensors.  No GPU compute."""
import ctypes as C
import os
import re

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model, net_model
from tests.test_ensemble_cpu import _members, _wrappers

ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED = -1, -2, -4
P = C.c_void_p(4096)
ES, EG, SG = 512, 256, 64
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'snsde.h')


def _solve(model, batch, members=0, samples=0, kernel='auto', method=0, flags=0, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method = model, batch, KNOTS, STEPS, 2, method
    s.members, s.samples = members, samples
    s.kernel, s.flags = _lib.KERNELS[kernel], flags
    if method == 2:
        s.srk_tab = P
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _train(s):
    s.traj = s.act_save = s.dW_out = P
    if s.method == 2:
        s.stage_save = s.dU_out = P
    return s


def _path(s):
    return _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(s))]


def _backward(s):
    b = _lib.Backward()
    b.fwd = s
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(b.fwd, f, P)
    b.grad_ys = b.adj = b.workspace = b.delta_save = P
    return b


def _answers(s):
    lib = _lib.lib()
    b = _backward(s)
    return (_path(s), engine.forward_kernel(s), engine.backward_kernel(s), int(lib.snsde_workspace_bytes(C.byref(s))),
            int(lib.snsde_backward_supported(C.byref(s))), int(lib.snsde_backward_workspace_bytes(C.byref(b))),
            int(lib.snsde_param_gradients_workspace_bytes(C.byref(b))))


def test_abi_is_unchanged_and_the_flag_is_512():
    lib = _lib.lib()
    assert _lib.FLAG_ENSEMBLE_SAMPLES == ES
    assert C.sizeof(_lib.Solve) == 304 and C.sizeof(_lib.Backward) == 368 and lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0
    assert re.search(r'SNSDE_FLAG_ENSEMBLE_SAMPLES\s*=\s*512', open(HEADER).read())


@pytest.mark.parametrize('members,samples,other', [(0, 0, 0), (1, 2, SG), (0, 2, SG), (3, 0, EG), (3, 1, EG), (1, 1, 0)])
def test_the_flag_alone_changes_nothing(members, samples, other):
    """members <= 1 or samples <= 1: path, kernel, workspaces and every backward answer are those without the flag, for inference
    and for training descriptors, with and without the opt-in that the other option has of its own."""
    for model in (elementwise_model(64), elementwise_model(128), net_model()):
        for kernel, method in (('auto', 0), ('mfma4', 1), ('mfma4', 2), ('auto', 2)):
            for train in (False, True):
                for extra in (0, other):
                    base = _solve(model, 24, members, samples, kernel, method, flags=extra)
                    flag = _solve(model, 24, members, samples, kernel, method, flags=extra | ES)
                    if train:
                        _train(base), _train(flag)
                    assert _answers(flag) == _answers(base), (members, samples, kernel, method, train, extra)


def test_the_flag_opens_the_combination_on_the_kernels_that_take_both():
    lib = _lib.lib()
    for H in (64, 128):
        model = elementwise_model(H)
        for kernel, method, fwd in (('auto', 0, 'lean'), ('auto', 1, 'lean'), ('mfma4', 0, 'lean'), ('mfma4', 2, 'general_m4'),
                                    ('auto', 2, 'general_m4')):
            on, off = _solve(model, 24, 3, 2, kernel, method, flags=ES), _solve(model, 24, 3, 2, kernel, method)
            assert _path(off) == 'none' and engine.forward_kernel(off) == 'none'
            assert _path(on) != 'none' and engine.forward_kernel(on) == fwd, (H, kernel, method)
            # the workspace is that of `members`: nothing per sample
            assert lib.snsde_workspace_bytes(C.byref(on)) == lib.snsde_workspace_bytes(C.byref(_solve(model, 24, 3, 0, kernel, method))) > 0
            # the member alone as a sampled shard runs the same kernel
            one = _solve(model, 8, 0, 2, kernel, method, row_offset=8, global_rows=24)
            assert engine.forward_kernel(one) == fwd
            assert lib.snsde_backward_supported(C.byref(on)) == 0      # (inference: no opt-in to training)
    assert _path(_solve(elementwise_model(64), 24, 3, 2, flags=ES)) == 'lean'
    assert _path(_solve(elementwise_model(64), 24, 3, 2, flags=ES | _lib.FLAG_BF16_OPERANDS)) == 'lean-bf16'
    assert engine.forward_path(elementwise_model(64), 24, KNOTS, STEPS, members=3, samples=2, ensemble_samples=True) == 'lean'
    assert engine.forward_path(elementwise_model(64), 24, KNOTS, STEPS, members=3, samples=2) == 'none'


def test_selectors_without_both_maps_stay_none():
    lib = _lib.lib()
    lean64 = elementwise_model(64)
    for s in (_solve(lean64, 24, 3, 2, 'generic', flags=ES), _solve(lean64, 96, 3, 2, 'mfma16', flags=ES),
              _solve(net_model(), 24, 3, 2, 'w4', flags=ES), _solve(net_model(), 24, 3, 2, 'auto', flags=ES),
              _solve(elementwise_model(256), 24, 3, 2, flags=ES), _solve(lean64, 24, 3, 2, 'generic', 2, flags=ES)):
        assert _path(s) == 'none' and engine.forward_kernel(s) == 'none'
        b = _backward(s)
        b.fwd.workspace_bytes = 1 << 30
        assert lib.snsde_solve_forward(C.byref(b.fwd), None) == ERR_UNSUPPORTED
    # what either option refuses on its own stays refused
    table = engine.model_struct(3, 64, 64, 2, 4, 13)
    for s in (_solve(lean64, 24, 3, 2, flags=ES, z0_weight=P, z0_bias=P), _solve(table, 24, 3, 2, flags=ES, noise_table=P),
              _solve(lean64, 24, 3, 2, flags=ES, kl_column1=3)):
        assert _path(s) == 'none'
        b = _backward(s)
        b.fwd.workspace_bytes = 1 << 30
        assert lib.snsde_solve_forward(C.byref(b.fwd), None) == ERR_UNSUPPORTED
    s = _solve(lean64, 24, 3, 2, flags=ES, params=P, coeffs=P, workspace=P)
    assert lib.snsde_eval_fg(C.byref(s), P, P, P, P, None) == ERR_UNSUPPORTED


def test_each_dimension_error():
    lib = _lib.lib()
    model = elementwise_model(64)
    bad = {'batch % M': _solve(model, 26, 3, 2, flags=ES), 'Bm % 4': _solve(model, 30, 3, 2, flags=ES),
           'Bm % S': _solve(model, 24, 3, 3, flags=ES), 'row_offset % S': _solve(model, 24, 3, 2, flags=ES, row_offset=1),
           'global_rows % S': _solve(model, 24, 3, 2, flags=ES, global_rows=25)}
    for what, s in bad.items():
        assert _path(s) == 'none', what
        assert lib.snsde_solve_forward(C.byref(s), None) == ERR_DIMS, what
        assert lib.snsde_backward_supported(C.byref(_train(s))) == 0, what
        b = _backward(s)
        b.fwd.flags = ES | EG | SG
        assert lib.snsde_solve_backward(C.byref(b), None) == ERR_DIMS, what
    # (the same descriptors with the dimensions right get past the dimension checks: the next complaint is the missing pointers)
    good = _solve(model, 24, 3, 2, flags=ES, row_offset=2, global_rows=26)
    assert _path(good) == 'lean' and lib.snsde_solve_forward(C.byref(good), None) == ERR_NULL
    # Bm % S is the flag's own check: without the flag the combination is unsupported, as before, whatever Bm is
    off = _backward(_solve(model, 24, 3, 3))
    off.fwd.workspace_bytes = 1 << 30
    assert lib.snsde_solve_forward(C.byref(off.fwd), None) == ERR_UNSUPPORTED


def test_training_needs_all_three_flags():
    lib = _lib.lib()
    for H in (64, 128):
        model = elementwise_model(H)
        for kernel, method, fwd, rev in (('auto', 0, 'lean', 'general'), ('auto', 1, 'lean', 'general'), ('mfma4', 0, 'lean', 'general'),
                                         ('auto', 2, 'general_m4', 'general_srk')):
            s = _train(_solve(model, 24, 3, 2, kernel, method, flags=ES | EG | SG))
            assert lib.snsde_backward_supported(C.byref(s)) == 1, (H, kernel, method)
            assert engine.forward_kernel(s) == fwd and engine.backward_kernel(s) == rev
            for pair in (ES | EG, ES | SG, EG | SG, ES, EG, SG, 0):
                t = _train(_solve(model, 24, 3, 2, kernel, method, flags=pair))
                assert lib.snsde_backward_supported(C.byref(t)) == 0, (pair, kernel, method)
                assert _path(t) == 'none' and engine.backward_kernel(t) == 'none', pair
                b = _backward(t)
                b.fwd.workspace_bytes = b.workspace_bytes = 1 << 30
                assert lib.snsde_solve_forward(C.byref(b.fwd), None) == ERR_UNSUPPORTED, pair
                assert lib.snsde_solve_backward(C.byref(b), None) == ERR_UNSUPPORTED, pair
                assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED, pair
                assert lib.snsde_param_gradients_workspace_bytes(C.byref(b)) == 0
            # each member is planned as its own sampled solve of Bm paths: the workspaces are M blocks of its own
            one = _train(_solve(model, 8, 0, 2, kernel, method, flags=SG, row_offset=8, global_rows=24))
            assert engine.forward_kernel(one) == fwd and engine.backward_kernel(one) == rev
            b, b1 = _backward(s), _backward(one)
            for query in (lib.snsde_backward_workspace_bytes, lib.snsde_param_gradients_workspace_bytes):
                alone = int(query(C.byref(b1)))
                assert alone > 0 and int(query(C.byref(b))) == 3 * ((alone + 15) & ~15), (query, alone)
            assert lib.snsde_coeff_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED
            assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(b)) == 0
    # coverage is that of ensemble_grad: nothing else gains an adjoint
    for s in (_solve(elementwise_model(64), 96, 3, 2, 'mfma16', flags=ES | EG | SG), _solve(net_model(), 24, 3, 2, 'mfma4', flags=ES | EG | SG),
              _solve(elementwise_model(256), 24, 3, 2, flags=ES | EG | SG), _solve(elementwise_model(64), 24, 3, 2, 'generic', flags=ES | EG | SG),
              _solve(elementwise_model(64), 24, 3, 2, flags=ES | EG | SG | _lib.FLAG_BF16_OPERANDS)):
        assert lib.snsde_backward_supported(C.byref(_train(s))) == 0 and _path(s) == 'none'
    grid = type('G', (), {'N': STEPS, 'T': 2})
    model = elementwise_model(64)
    kw = dict(members=3, samples=2)
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', ensemble_samples=True, ensemble_grad=True, sample_grad=True, **kw) == 1
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', ensemble_samples=True, ensemble_grad=True, **kw) == 0
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', ensemble_samples=True, sample_grad=True, **kw) == 0
    assert engine.backward_mode(model, 24, KNOTS, grid, 'euler', ensemble_grad=True, sample_grad=True, **kw) == 0
    assert engine.forward_path(model, 24, KNOTS, STEPS, training=True, ensemble_samples=True, ensemble_grad=True, sample_grad=True, **kw) == 'lean'


def test_the_two_statistics_exports_are_declared_bound_and_validate_first():
    lib = _lib.lib()
    header = open(HEADER).read()
    for name in ('snsde_ensemble_stats', 'snsde_ensemble_stats_backward'):
        assert name in _lib.EXPORTS and re.search(r'^SNSDE_API\s+int\s+' + name + r'\s*\(', header, re.M)
        assert getattr(lib, name).argtypes is not None
    f, b = lib.snsde_ensemble_stats, lib.snsde_ensemble_stats_backward
    # forward: (ys, outer, M, G, S, W, mean, within, between, stream)
    assert f(None, 1, 2, 3, 2, 4, P, P, P, None) == ERR_NULL
    for dims in ((0, 2, 3, 2, 4), (1, 0, 3, 2, 4), (1, 2, 0, 2, 4), (1, 2, 3, 0, 4), (1, 2, 3, 2, 0), (1, 2, 3, -1, 4),
                 (1 << 40, 2, 1 << 40, 2, 4)):
        assert f(P, *dims, P, P, P, None) == ERR_DIMS, dims
    assert f(P, 1, 2, 3, 1, 4, P, P, None, None) == ERR_DIMS      # within divides by S - 1
    assert f(P, 1, 1, 3, 2, 4, P, None, P, None) == ERR_DIMS      # between divides by M - 1
    assert f(P, 1, 2, 3, 2, 4, None, None, None, None) == 0       # nothing wanted: nothing launched
    # backward: (grad_mean, grad_within, grad_between, ys, outer, M, G, S, W, grad_ys, stream)
    assert b(P, None, None, None, 1, 2, 3, 2, 4, None, None) == ERR_NULL
    assert b(P, P, None, None, 1, 2, 3, 2, 4, P, None) == ERR_NULL      # a variance term reads ys
    assert b(P, None, P, None, 1, 2, 3, 2, 4, P, None) == ERR_NULL
    assert b(P, None, None, None, 1, 2, 0, 2, 4, P, None) == ERR_DIMS
    assert b(P, P, None, P, 1, 2, 3, 1, 4, P, None) == ERR_DIMS
    assert b(P, None, P, P, 1, 1, 3, 2, 4, P, None) == ERR_DIMS


# ---- front end on CPU tensors ---------------------------------------------------------------------------------------------------

def test_option_checks():
    sdes, y0, times = _members()
    ts = torch.tensor([0., 2.2, 5.])
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='ensemble_samples must be a bool'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'samples': 2, 'ensemble_samples': bad})
        with pytest.raises(ValueError, match='ensemble_samples must be a bool'):
            engine.check_ensemble_samples(bad)
    assert engine.check_ensemble_samples(True) is True and engine.check_ensemble_samples(False) is False
    with pytest.raises(ValueError, match='samples'):      # no opt-in: as before
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'samples': 2})
    with pytest.raises(ValueError, match='samples'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'samples': 2, 'ensemble_samples': False})
    for opt in ({'sample_grad': True}, {'sample_grad': True, 'ensemble_samples': True}, {'sample_grad': True, 'samples': 1, 'ensemble_samples': True}):
        with pytest.raises(ValueError, match='sample_grad'):      # sample_grad without samples > 1 and the opt-in: as before
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options=opt)
        with pytest.raises(ValueError, match='sample_grad'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options=dict(opt, ensemble_grad=True))
    ya = y0.clone().requires_grad_(True)
    es = {'samples': 2, 'ensemble_samples': True}
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=0.5, options=es)
    with pytest.raises(ValueError, match='sample_grad'):
        S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=0.5, options=dict(es, ensemble_grad=True))
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=0.5, options=dict(es, sample_grad=True))
    with pytest.raises(ValueError, match='multiples of samples'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options=dict(es, row_offset=1, global_rows=26))
    with pytest.raises(ValueError, match='rows per member'):
        S.sdeint_ensemble(sdes, y0[:, :3], ts, method='euler', dt=0.5, options=es)
    with pytest.raises(NotImplementedError, match='strict'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options=dict(es, strict=True))
    # SolveCall checks its arguments before it touches the device
    model = elementwise_model(64)
    with pytest.raises(ValueError, match='inference only'):
        engine.SolveCall(model, torch.zeros(3, 8), torch.zeros(4, KNOTS - 1, 12), None, torch.zeros(24, 64), members=3, samples=2)
    with pytest.raises(ValueError, match='groups of `samples`'):
        engine.SolveCall(model, torch.zeros(3, 8), torch.zeros(4, KNOTS - 1, 12), None, torch.zeros(24, 64), members=3, samples=3,
                         ensemble_samples=True)


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_cpu_ensemble_samples_equal_the_sampled_calls(method):
    sdes, y0, times = _members()      # M = 3, B = 4 input rows, H = 16
    M, B, Sn = 3, 4, 3
    ts = torch.tensor([0., 1.3, 2.2, 5.])
    opts = {'seed': 11, 'samples': Sn, 'ensemble_samples': True}
    with torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=opts)
        ref = torch.stack([S.sdeint(sde, y0[m], ts, method=method, dt=0.5,
                                    options={'seed': 11, 'samples': Sn, 'row_offset': m * B * Sn, 'global_rows': M * B * Sn})
                           for m, sde in enumerate(sdes)], dim=1)
        assert tuple(got.shape) == (4, M, B * Sn, 16) and torch.equal(got, ref)
        # y0 already one row per path, a shard of a larger problem, row_out of either length
        wide = y0.repeat_interleave(Sn, dim=1)
        assert torch.equal(S.sdeint_ensemble(sdes, wide, ts, method=method, dt=0.5, options=opts), got)
        sh = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=dict(opts, row_offset=6, global_rows=60))
        ref = torch.stack([S.sdeint(sde, y0[m], ts, method=method, dt=0.5,
                                    options={'seed': 11, 'samples': Sn, 'row_offset': 6 + m * B * Sn, 'global_rows': 60})
                           for m, sde in enumerate(sdes)], dim=1)
        assert torch.equal(sh, ref)
        ro = torch.tensor([3, 0, 2, 1])
        a = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=dict(opts, row_out=ro))
        b = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=dict(opts, row_out=ro.repeat_interleave(Sn)))
        assert tuple(a.shape) == (M, B * Sn, 16) and torch.equal(a, b)
        idx = ro.repeat_interleave(Sn).reshape(1, 1, -1, 1).expand(1, M, B * Sn, 16)
        assert torch.equal(a, got.gather(0, idx).squeeze(0))
    # the paths of one input row differ from each other, and the members differ
    paths = got[-1].reshape(M, B, Sn, 16)
    assert (paths[:, :, 0] - paths[:, :, 1]).abs().max() > 1e-4 and (got[-1, 0] - got[-1, 1]).abs().max() > 1e-4


def test_cpu_training_equals_the_loop_of_sampled_differentiable_solves():
    sdes, y0, times = _members()
    for sde in sdes:
        sde.requires_grad_(True)
    M, B, Sn = 3, 4, 2
    ts = torch.tensor([0., 1.3, 2.2, 5.])
    cot = torch.randn(4, M, B * Sn, 16, generator=torch.Generator().manual_seed(2))
    ya = y0.clone().requires_grad_(True)
    got = S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=0.5,
                            options={'seed': 11, 'samples': Sn, 'ensemble_samples': True, 'ensemble_grad': True, 'sample_grad': True})
    (got * cot).sum().backward()
    mine = [[p.grad.clone() for p in sde.parameters()] for sde in sdes]
    for sde in sdes:
        sde.zero_grad(set_to_none=True)
    yb = y0.clone().requires_grad_(True)
    ref = torch.stack([S.sdeint(sde, yb[m], ts, method='euler', dt=0.5,
                                options={'seed': 11, 'samples': Sn, 'sample_grad': True, 'row_offset': m * B * Sn, 'global_rows': M * B * Sn})
                       for m, sde in enumerate(sdes)], dim=1)
    (ref * cot).sum().backward()
    assert torch.equal(got, ref) and torch.equal(ya.grad, yb.grad) and ya.grad.abs().max() > 0
    for gm, sde in zip(mine, sdes):
        assert all(torch.equal(a, p.grad) for a, p in zip(gm, sde.parameters())) and any(a.abs().max() > 0 for a in gm)
        sde.zero_grad(set_to_none=True)
        sde.requires_grad_(False)


def test_cpu_ensemble_module_passes_the_options_through():
    models, coeffs, times = _wrappers(S.NeuralSDE)
    M, B, Sn = len(models), coeffs.shape[0], 2
    ens = S.Ensemble(models).eval()
    fi = torch.tensor([5, 3, 5, 2])
    with torch.no_grad():
        got = ens(times, (coeffs,), fi, options={'seed': 7, 'samples': Sn, 'ensemble_samples': True})
        refs = [net(times, (coeffs,), fi, options={'seed': 7, 'samples': Sn, 'row_offset': m * B * Sn, 'global_rows': M * B * Sn})
                for m, net in enumerate(models)]
    assert tuple(got.shape) == (M, B * Sn, 3) and torch.equal(got, torch.stack(refs))


@pytest.mark.parametrize('kind', [S.NeuralSDE, S.IstsNeuralSDE])
def test_cpu_ensemble_module_trains_through_sample_paths_like_the_wrappers(kind):
    models, coeffs, times = _wrappers(kind)
    M, B, Sn = len(models), coeffs.shape[0], 2
    for net in models:
        net.train().requires_grad_(True)
    ens = S.Ensemble(models).train()
    fi = torch.tensor([5, 3, 5, 2])
    args = (coeffs, times) if kind is S.IstsNeuralSDE else (times, (coeffs,), fi)
    first = (lambda o: o[0]) if kind is S.IstsNeuralSDE else (lambda o: o)
    torch.manual_seed(123)      # (the classification head's Dropout draws per member, in member order in both arms)
    got = first(ens(*args, options={'seed': 7, 'samples': Sn, 'ensemble_samples': True, 'ensemble_grad': True, 'sample_grad': True}))
    assert got.shape[:2] == (M, B * Sn)
    cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(1))
    (got * cot).sum().backward()
    mine = [[p.grad.clone() for p in net.parameters()] for net in models]
    for net in models:
        net.zero_grad(set_to_none=True)
    torch.manual_seed(123)
    refs = torch.stack([first(net(*args, options={'seed': 7, 'samples': Sn, 'sample_grad': True, 'row_offset': m * B * Sn,
                                                  'global_rows': M * B * Sn})) for m, net in enumerate(models)])
    (refs * cot).sum().backward()
    assert torch.equal(got, refs)
    for gm, net in zip(mine, models):
        assert all(torch.equal(a, p.grad) for a, p in zip(gm, net.parameters()))
        assert any(a.abs().max() > 0 for a in gm)
        net.zero_grad(set_to_none=True)
    with pytest.raises(ValueError):
        ens(*args, options={'seed': 7, 'samples': Sn, 'ensemble_samples': True, 'ensemble_grad': True})


@pytest.mark.parametrize('shape', [(2, 3, 5, 4, 8), (1, 2, 3, 2, 7), (1, 4, 1, 3, 1)])
def test_ensemble_stats_on_cpu_tensors_against_float64(shape):
    O, M, G, Sn, W = shape
    x = torch.randn(O, M, G * Sn, W, generator=torch.Generator().manual_seed(3)) + 0.5
    mean, within, between = S.ensemble_stats(x, M, Sn)
    v = x.double().reshape(O, M, G, Sn, W)
    mm = v.mean(dim=3)
    assert tuple(mean.shape) == tuple(within.shape) == tuple(between.shape) == (O, G, W) and mean.dtype == torch.float32
    assert torch.allclose(mean.double(), mm.mean(dim=1), rtol=0, atol=1e-6)
    assert torch.allclose(within.double(), v.var(dim=3, unbiased=True).mean(dim=1), rtol=1e-5, atol=1e-6)
    assert torch.allclose(between.double(), mm.var(dim=1, unbiased=True), rtol=1e-5, atol=1e-6)
    # per member it is sample_stats, and the law of total variance holds for the two parts: with equal group sizes
    # (M S - 1) var_all = M (S - 1) within + S (M - 1) between
    for m in range(M):
        sm, sv = S.sample_stats(x[:, m], Sn)
        assert torch.allclose(sm.double(), mm[:, m], rtol=0, atol=1e-6)
    pooled = v.permute(0, 2, 1, 3, 4).reshape(O, G, M * Sn, W).var(dim=2, unbiased=True)
    assert torch.allclose((M * Sn - 1) * pooled, M * (Sn - 1) * within.double() + Sn * (M - 1) * between.double(), rtol=1e-4, atol=1e-5)
    # float64 input stays float64; the optional outputs; autograd through the tensor-op form
    m64, w64, b64 = S.ensemble_stats(x.double(), M, Sn, between=False)
    assert m64.dtype == torch.float64 and b64 is None and torch.allclose(w64, v.var(dim=3, unbiased=True).mean(dim=1))
    assert S.ensemble_stats(x, M, Sn, within=False)[1] is None
    xa = x.double().clone().requires_grad_(True)
    a, b, c = S.ensemble_stats(xa, M, Sn)
    (a.sum() + 2 * b.sum() + 3 * c.sum()).backward()
    assert xa.grad is not None and torch.isfinite(xa.grad).all()
    with pytest.raises(ValueError):
        S.ensemble_stats(x, M + 1, Sn)
    with pytest.raises(ValueError):
        S.ensemble_stats(x[:, :, :G * Sn - 1], M, Sn)
    if Sn == 2:
        with pytest.raises(ValueError, match='samples >= 2'):
            S.ensemble_stats(x, M, 1)
    with pytest.raises(ValueError, match='members >= 2'):
        S.ensemble_stats(x[:, :1], 1, Sn)
