"""options={'samples': S, 'sample_grad': True} / SNSDE_FLAG_SAMPLE_GRAD on the host: the flag's place in the C ABI, what the
library plans for a sampled training descriptor and what it still refuses, the entry points' validation order (dummy pointers:
every check happens before a buffer is touched), and the option on CPU tensors, where it differentiates through the replicated
tensor-op loop.  No GPU compute."""
import ctypes as C

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model, net_model
from tests.golden.make_route_golden import ANSWERS, FIELDS, answers, solve_struct
from tests.helpers import load, make_problem

ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4, -5
P = C.c_void_p(4096)
FLAG = 64


def _solve(model, batch, samples=0, kernel='auto', method=0, flags=FLAG, train=True, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method, s.samples = model, batch, KNOTS, STEPS, 2, method, samples
    s.kernel, s.flags = _lib.KERNELS[kernel], flags
    if method == 2:
        s.srk_tab = P
    if train:      # what a training forward writes
        s.traj = s.act_save = s.dW_out = P
        if method == 2:
            s.stage_save = s.dU_out = P
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _path(s):
    return _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(s))]


def _mode(s):
    return _lib.lib().snsde_backward_supported(C.byref(s))


def _fill(s):
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(s, f, P)
    return s


def _launch_rc(s, workspace_bytes=0):
    s.workspace_bytes = workspace_bytes
    return _lib.lib().snsde_solve_forward(C.byref(_fill(s)), None)


def _backward(s):
    b = _lib.Backward()
    b.fwd = _fill(s)
    b.fwd.workspace_bytes = 1 << 30
    return b


# ---- C ABI ------------------------------------------------------------------------------------------------------------------

def test_the_flag_is_64_and_no_struct_changed():
    lib = _lib.lib()
    assert _lib.FLAG_SAMPLE_GRAD == FLAG
    header = open(__file__.rsplit('/tests/', 1)[0] + '/include/snsde.h').read()
    assert 'SNSDE_FLAG_SAMPLE_GRAD = 64' in header
    assert [f[0] for f in _lib.Solve._fields_][-3:] == ['global_rows', 'samples', 'reserved3']
    assert [f[0] for f in _lib.Backward._fields_] == ['struct_size', 'fwd', 'grad_ys', 'adj', 'delta_save', 'workspace', 'workspace_bytes',
                                                     'grad_noise_table', 'flags', 'reserved']
    assert (C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward)) == (40, 304, 368)      # (as on the parent commit)
    assert lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0
    assert _launch_rc(_solve(elementwise_model(64), 12, 3, reserved3=1)) == ERR_DIMS      # reserved3 stays "must be 0"


def test_covered_descriptors_plan_a_forward_and_the_mfma_adjoint():
    lean = elementwise_model(64)
    for H in (32, 64, 128):
        m = elementwise_model(H)
        assert _path(_solve(m, 12, 3, 'mfma4')) == 'lean' and _mode(_solve(m, 12, 3, 'mfma4')) == 1, H
    assert _path(_solve(elementwise_model(128), 12, 3)) == 'lean' and _mode(_solve(elementwise_model(128), 12, 3)) == 1
    lg = FLAG | _lib.FLAG_LEAN_GENERAL
    assert _path(_solve(elementwise_model(128), 12, 3, flags=lg)) == 'lean' and _mode(_solve(elementwise_model(128), 12, 3, flags=lg)) == 1
    for method in (0, 1):
        assert _path(_solve(lean, 35, 7, 'mfma16', method)) == 'mfma16' and _mode(_solve(lean, 35, 7, 'mfma16', method)) == 1
        assert _mode(_solve(lean, 12, 3, 'mfma4', method)) == 1
    assert _path(_solve(lean, 12, 3, 'mfma4', 2)) == 'mfma-srk' and _mode(_solve(lean, 12, 3, 'mfma4', 2)) == 1
    assert _path(_solve(lean, 35, 7, 'mfma16', 2)) == 'mfma-srk' and _mode(_solve(lean, 35, 7, 'mfma16', 2)) == 1
    # the launch gets past the validation (stops at the workspace size)
    assert _launch_rc(_solve(lean, 12, 3, 'mfma4')) == ERR_WORKSPACE
    # without the flag: exactly as before
    assert _path(_solve(lean, 12, 3, 'mfma4', flags=0)) == 'none' and _mode(_solve(lean, 12, 3, 'mfma4', flags=0)) == 0
    assert _launch_rc(_solve(lean, 12, 3, 'mfma4', flags=0)) == ERR_UNSUPPORTED
    assert engine.backward_mode(lean, 12, KNOTS, type('G', (), {'N': STEPS, 'T': 2}), 'euler', 'mfma4', samples=3, sample_grad=True) == 1
    assert engine.backward_mode(lean, 12, KNOTS, type('G', (), {'N': STEPS, 'T': 2}), 'euler', 'mfma4', samples=3) == 0
    assert engine.forward_path(lean, 12, KNOTS, STEPS, kernel='mfma4', samples=3, sample_grad=True, training=True) == 'lean'
    assert engine.forward_path(lean, 12, KNOTS, STEPS, kernel='mfma4', samples=3, training=True) == 'none'


def test_uncovered_descriptors_are_no_plan_and_never_another_kernel():
    lean, net, h256 = elementwise_model(64), net_model(), elementwise_model(256)
    wide = engine.model_struct(3, 48, 48, 2, 4, 17)      # no MFMA instantiation: `auto` would arrive at the generic family
    for what, s in (('generic', _solve(lean, 12, 3, 'generic')), ('generic srk', _solve(lean, 12, 3, 'generic', 2)),
                    ('auto -> generic', _solve(wide, 12, 3)), ('wave pairs', _solve(net, 12, 3)), ('w4', _solve(net, 12, 3, 'w4')),
                    ('net, 4-row tiles', _solve(net, 12, 3, 'mfma4')), ('net srk', _solve(net, 12, 3, method=2)),
                    ('net milstein', _solve(net, 12, 3, method=1)), ('H = 256', _solve(h256, 12, 3)),
                    ('H = 256 mfma16', _solve(h256, 35, 7, 'mfma16')), ('kl column', _solve(lean, 12, 3, 'mfma4', kl_column1=3))):
        assert _mode(s) == 0, what
        assert _path(s) == 'none', what      # (also where a forward kernel maps paths - H = 256 on 16-row tiles, a net on 4-row tiles:
        assert _launch_rc(s, 1 << 30) == ERR_UNSUPPORTED, what      #  training planes no sampled adjoint would read are refused)
        b = _backward(s)
        b.grad_ys = b.adj = b.workspace = b.delta_save = P
        b.workspace_bytes = 1 << 30
        lib = _lib.lib()
        assert lib.snsde_param_gradients_workspace_bytes(C.byref(b)) == 0, what
        assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(b)) == 0, what
        if what != 'kl column':
            assert lib.snsde_solve_backward(C.byref(b), None) == ERR_UNSUPPORTED, what
            assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED, what
            assert lib.snsde_param_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED, what
            assert lib.snsde_coeff_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED, what


def test_initial_state_probe_and_bf16_stay_refused():
    lib = _lib.lib()
    lean = elementwise_model(64)
    s = _solve(lean, 12, 3, 'mfma4', z0_weight=P, z0_bias=P)
    assert _path(s) == 'none' and _launch_rc(s) == ERR_UNSUPPORTED
    s = _solve(lean, 12, 3, 'mfma4', train=False, z0_weight=P, z0_bias=P)
    assert _path(s) == 'none' and _launch_rc(s) == ERR_UNSUPPORTED
    for samples, want in ((3, ERR_UNSUPPORTED), (0, ERR_WORKSPACE)):
        s = _solve(lean, 12, samples, train=False, params=P, coeffs=P, workspace=P)
        assert lib.snsde_eval_fg(C.byref(s), P, P, P, P, None) == want
    h128 = elementwise_model(128)
    bf = FLAG | _lib.FLAG_BF16_OPERANDS
    assert _path(_solve(h128, 12, 3, train=False, flags=_lib.FLAG_BF16_OPERANDS)) == 'lean-bf16'
    for train in (False, True):
        s = _solve(h128, 12, 3, train=train, flags=bf)
        assert _path(s) == 'none' and _mode(s) == 0 and _launch_rc(s, 1 << 30) == ERR_UNSUPPORTED
    # no effect without samples: the bf16 inference solve is the one it was
    assert _path(_solve(h128, 12, 0, train=False, flags=bf)) == _path(_solve(h128, 12, 1, train=False, flags=bf)) == 'lean-bf16'


def test_the_flag_with_zero_or_one_sample_changes_no_answer_of_the_route_fixture():
    g = load('routes.npz')
    assert tuple(g['fields']) == FIELDS
    lib = _lib.lib()
    n = 0
    for row in g['desc'][::3]:
        base = answers(row)
        for samples in (0, 1):
            s = solve_struct(row)
            s.samples = samples
            s.flags |= FLAG
            b = _lib.Backward()
            b.fwd = s
            assert [lib.snsde_forward_path(C.byref(s)), lib.snsde_backward_supported(C.byref(s)), lib.snsde_workspace_bytes(C.byref(s)),
                    lib.snsde_backward_workspace_bytes(C.byref(b))] == base[:4], (row, samples)
            n += 1
    assert n > 400 and ANSWERS[0] == 'forward_path'


def test_save_layout_and_workspaces_are_those_of_the_replicated_descriptor():
    lib = _lib.lib()
    for model, batch, Sn, kernel, method in ((elementwise_model(64), 12, 3, 'mfma4', 0), (elementwise_model(128), 12, 3, 'auto', 1),
                                             (elementwise_model(64), 35, 7, 'mfma16', 0), (elementwise_model(64), 12, 3, 'mfma4', 2)):
        lay = []
        for s in (_solve(model, batch, Sn, kernel, method), _solve(model, batch, 0, kernel, method, flags=0)):
            a, p, d = C.c_int32(), C.c_int32(), C.c_int32()
            assert lib.snsde_save_layout(C.byref(s), C.byref(a), C.byref(p), C.byref(d)) == 0
            b = _backward(s)
            lay.append((a.value, p.value, d.value, lib.snsde_backward_workspace_bytes(C.byref(b)),
                        lib.snsde_param_gradients_workspace_bytes(C.byref(b)), lib.snsde_coeff_gradients_workspace_bytes(C.byref(b))))
        assert lay[0] == lay[1] and lay[0][2] > 0 and min(lay[0][3:]) > 0, (kernel, method, lay)
    # the coefficient-gradient workspace holds v for `batch` PATHS: M (H C, padded to 64 floats) + passes x batch x C + 64 floats
    m = elementwise_model(64)
    Cn, H = m.input_channels, m.hidden_channels
    want = (((H * Cn + 63) // 64) * 64 + STEPS * 12 * Cn + 64) * 4
    assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(_backward(_solve(m, 12, 3, 'mfma4')))) == want
    assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(_backward(_solve(m, 12, 3, 'mfma4', flags=0)))) == 0


def test_every_backward_entry_point_validates_before_it_touches_a_buffer():
    lib = _lib.lib()
    lean = elementwise_model(64)

    def fresh(**kw):
        b = _backward(_solve(lean, 12, 3, 'mfma4', **kw))
        b.grad_ys = b.adj = b.workspace = b.delta_save = P
        b.workspace_bytes = 1 << 30
        return b
    b = fresh()
    b.workspace_bytes = 16
    assert lib.snsde_solve_backward(C.byref(b), None) == ERR_WORKSPACE
    assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_WORKSPACE
    assert lib.snsde_param_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_WORKSPACE
    b = fresh()
    assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 16, None) == ERR_WORKSPACE
    assert lib.snsde_param_gradients(C.byref(b), P, P, 16, None) == ERR_WORKSPACE
    assert lib.snsde_coeff_gradients(C.byref(b), P, P, 16, None) == ERR_WORKSPACE
    assert lib.snsde_coeff_gradients(C.byref(b), None, P, 1 << 30, None) == ERR_NULL
    assert lib.snsde_param_gradients(C.byref(b), None, P, 1 << 30, None) == ERR_NULL
    assert lib.snsde_backward_with_gradients(C.byref(b), P, None, 1 << 30, None) == ERR_NULL
    b.grad_ys = None
    assert lib.snsde_solve_backward(C.byref(b), None) == ERR_NULL
    assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_NULL
    b = fresh()
    b.delta_save = None
    assert lib.snsde_param_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_NULL
    assert lib.snsde_coeff_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_UNSUPPORTED      # (no planes: as for one path per row)
    b = fresh(traj=None)
    assert lib.snsde_solve_backward(C.byref(b), None) == ERR_NULL
    b = fresh()
    b.fwd.batch = 13      # not whole groups
    assert lib.snsde_solve_backward(C.byref(b), None) == ERR_DIMS and lib.snsde_coeff_gradients(C.byref(b), P, P, 1 << 30, None) == ERR_DIMS


def test_the_stats_backward_is_exported_declared_bound_and_validates():
    lib = _lib.lib()
    header = open(__file__.rsplit('/tests/', 1)[0] + '/include/snsde.h').read()
    assert 'SNSDE_API int snsde_sample_stats_backward(' in header
    assert 'snsde_sample_stats_backward' in _lib.EXPORTS and hasattr(lib, 'snsde_sample_stats_backward')
    f = lib.snsde_sample_stats_backward
    assert f(None, P, P, P, 1, 2, 1, P, None) == ERR_NULL and f(P, P, P, P, 1, 2, 1, None, None) == ERR_NULL
    assert f(P, P, None, P, 1, 2, 1, P, None) == ERR_NULL and f(P, P, P, None, 1, 2, 1, P, None) == ERR_NULL
    assert f(P, None, None, None, 0, 2, 1, P, None) == ERR_DIMS and f(P, None, None, None, 1, 0, 1, P, None) == ERR_DIMS
    assert f(P, None, None, None, 1, 2, 0, P, None) == ERR_DIMS
    assert f(P, P, P, P, 1, 1, 4, P, None) == ERR_DIMS      # the variance of one sample has no gradient either


# ---- Python on CPU tensors ----------------------------------------------------------------------------------------------------

def _model(dtype=torch.float64, B=4, H=16, C_=3, L=6, io=4, no=17, seed=5):
    pr = make_problem(seed, io, no, 2, B, H, C_, L, times=np.array([0., 0.7, 1.9, 2.4, 4.1, 5.][:L], np.float32))
    m = S.Diffusion_model(C_, H, H, 2, input_option=io, noise_option=no)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(dtype)
    coeffs = torch.from_numpy(pr['coeffs']).to(dtype).requires_grad_(True)
    m.set_X(coeffs, torch.from_numpy(pr['times']).to(dtype))
    return m, pr, coeffs, torch.from_numpy(pr['y0']).to(dtype).requires_grad_(True)


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_sample_grad_differentiates_through_the_replicated_tensor_op_loop(method):
    Sn = 3
    m, pr, coeffs, y0 = _model()
    ts = torch.from_numpy(pr['times']).double()
    w = torch.from_numpy(np.random.default_rng(3).standard_normal((len(ts), Sn * pr['B'], pr['H'])))
    ys = S.sdeint(m, y0, ts, dt=0.5, method=method, options={'samples': Sn, 'sample_grad': True, 'seed': 11})
    assert tuple(ys.shape) == (len(ts), Sn * pr['B'], pr['H']) and m.coeffs is coeffs
    (ys * w).sum().backward()
    got = dict(y0=y0.grad.clone(), coeffs=coeffs.grad.clone(), **{n: p.grad.clone() for n, p in m.named_parameters()})
    assert tuple(got['coeffs'].shape) == tuple(coeffs.shape) and tuple(got['y0'].shape) == tuple(y0.shape)
    # by hand: replicate, solve, and let autograd sum over the paths
    m2, _, coeffs2, y02 = _model()
    m2.set_X(coeffs2.repeat_interleave(Sn, 0), m2.times)
    ref = S.sdeint(m2, y02.repeat_interleave(Sn, 0), ts, dt=0.5, method=method, options={'seed': 11})
    assert torch.equal(ys.detach(), ref.detach())
    (ref * w).sum().backward()
    assert torch.allclose(got['y0'], y02.grad, rtol=1e-12, atol=1e-12) and float(y02.grad.abs().max()) > 0
    assert torch.allclose(got['coeffs'], coeffs2.grad, rtol=1e-12, atol=1e-12) and float(coeffs2.grad.abs().max()) > 0
    for n, p in m2.named_parameters():
        assert torch.allclose(got[n], p.grad, rtol=1e-12, atol=1e-12), n
    # y0 given per path: its gradient is per path
    m3, _, coeffs3, y03 = _model()
    y0p = y03.detach().repeat_interleave(Sn, 0).requires_grad_(True)
    ys3 = S.sdeint(m3, y0p, ts, dt=0.5, method=method, options={'samples': Sn, 'sample_grad': True, 'seed': 11})
    (ys3 * w).sum().backward()
    assert tuple(y0p.grad.shape) == (Sn * pr['B'], pr['H'])
    assert torch.allclose(y0p.grad.reshape(pr['B'], Sn, -1).sum(1), y02.grad, rtol=1e-12, atol=1e-12)


def test_option_validation():
    m, pr, coeffs, y0 = _model()
    ts = torch.from_numpy(pr['times']).double()
    for bad in (1, 0, 'yes', None, 1.0):
        with pytest.raises(ValueError, match='sample_grad'):
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 2, 'sample_grad': bad})
        with pytest.raises(ValueError, match='sample_grad'):      # (checked with or without samples)
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'sample_grad': bad})
    for opt in ({'recompute': 2}, {'save_traj': True}, {'precision': 'bf16'}, {'param_pass': 'torch'}):
        with pytest.raises(ValueError, match='sample_grad'):
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options=dict(opt, samples=2, sample_grad=True))
    # without the opt-in, and with sample_grad=False: the refusal of before
    for opt in ({}, {'sample_grad': False}):
        with pytest.raises(ValueError, match='inference only'):
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options=dict(opt, samples=2))
    # no effect on one path per row
    a = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 1, 'sample_grad': True, 'seed': 4})
    b = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'sample_grad': True, 'seed': 4})
    c = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'seed': 4})
    assert torch.equal(a, c) and torch.equal(b, c) and a.requires_grad


def test_sample_stats_on_cpu_tensors_keeps_the_tensor_op_statement_and_its_graph():
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 12, 5))).requires_grad_(True)
    mean, var = S.sample_stats(x, 3)
    assert mean.grad_fn is not None and 'SampleStats' not in type(mean.grad_fn).__name__
    (mean.sum() + (var * var).sum()).backward()
    ref = x.detach().clone().requires_grad_(True)
    v = ref.reshape(2, 4, 3, 5)
    (v.mean(2).sum() + (v.var(2) ** 2).sum()).backward()
    assert torch.allclose(x.grad, ref.grad, rtol=1e-12, atol=1e-12)


def test_wrapper_in_training_mode_returns_one_readout_row_per_path():
    m, pr, coeffs, _ = _model(torch.float32)
    net = S.NeuralSDE(m, pr['C'], pr['H'], 2).train()
    out = net(torch.from_numpy(pr['times']), (coeffs,), torch.tensor([5, 3, 5, 2]), options={'samples': 3, 'sample_grad': True, 'seed': 2})
    assert tuple(out.shape) == (3 * pr['B'], 2)
    out.square().sum().backward()
    assert tuple(coeffs.grad.shape) == tuple(coeffs.shape) and bool(torch.isfinite(coeffs.grad).all()) and float(coeffs.grad.abs().max()) > 0
    assert float(net.initial_network.weight.grad.abs().max()) > 0
    with pytest.raises(ValueError, match='inference only'):
        net(torch.from_numpy(pr['times']), (coeffs,), torch.tensor([5, 3, 5, 2]), options={'samples': 3, 'seed': 2})
