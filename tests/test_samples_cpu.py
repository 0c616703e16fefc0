"""options={'samples': S} / snsde_solve::samples on the host: option validation, the tensor-op backend against hand-replicated
coefficients, the grown C struct and its host-only queries, and sample_stats on CPU tensors.  No GPU compute."""
import ctypes as C

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model, net_model
from tests.golden.make_route_golden import ANSWERS, FIELDS, answers, solve_struct
from tests.helpers import load, make_problem

ERR_DIMS, ERR_UNSUPPORTED = -2, -4


def _model(B=4, H=16, C_=3, L=6, io=4, no=17, seed=5):
    pr = make_problem(seed, io, no, 2, B, H, C_, L, times=np.array([0., 0.7, 1.9, 2.4, 4.1, 5.][:L], np.float32))
    m = S.Diffusion_model(C_, H, H, 2, input_option=io, noise_option=no)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.from_numpy(pr['params'][name]))
    m.requires_grad_(False)
    m.set_X(torch.from_numpy(pr['coeffs']), torch.from_numpy(pr['times']))
    return m, pr


@pytest.mark.parametrize('bad', [0, -1, 2.5, '4', True])
@pytest.mark.parametrize('backend', ['auto', 'torch'])
def test_samples_must_be_a_positive_integer(bad, backend):
    m, pr = _model()
    ts = torch.from_numpy(pr['times'])
    with pytest.raises(ValueError, match='samples'):
        S.sdeint(m, torch.from_numpy(pr['y0']), ts, dt=1.0, method='euler', options={'samples': bad, 'backend': backend})


def test_samples_is_inference_only():
    m, pr = _model()
    ts, y0 = torch.from_numpy(pr['times']), torch.from_numpy(pr['y0'])
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint(m, y0.clone().requires_grad_(True), ts, dt=1.0, method='euler', options={'samples': 2})
    m.requires_grad_(True)
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 2})
    with torch.no_grad():      # (no autograd: accepted)
        assert S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 2, 'seed': 1}).shape[1] == 2 * y0.shape[0]
    m.requires_grad_(False)
    for opt in ({'save_traj': True}, {'recompute': 2}):
        with pytest.raises(ValueError, match='inference only'):
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options=dict(opt, samples=2))
    with pytest.raises(ValueError, match='rows'):
        S.sdeint(m, y0[:3], ts, dt=1.0, method='euler', options={'samples': 2})
    with pytest.raises(ValueError, match='row_offset'):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 2, 'row_offset': 3})


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_tensor_backend_samples_equal_the_hand_replicated_solve(method):
    """(T, 3B, H), equal to the call with y0 and the coefficients replicated by hand under the same seed, and the paths of one
    input row differ.  Without the feature the option is ignored and the result is (T, B, H)."""
    m, pr = _model()
    B, H, Sn = pr['B'], pr['H'], 3
    ts, y0 = torch.from_numpy(pr['times']), torch.from_numpy(pr['y0'])
    coeffs = m.coeffs
    got = S.sdeint(m, y0, ts, dt=0.5, method=method, options={'samples': Sn, 'seed': 11, 'backend': 'torch'})
    assert tuple(got.shape) == (len(ts), Sn * B, H)
    assert m.coeffs is coeffs      # the module's control path is put back
    m.set_X(coeffs.repeat_interleave(Sn, 0), m.times)
    ref = S.sdeint(m, y0.repeat_interleave(Sn, 0), ts, dt=0.5, method=method, options={'seed': 11, 'backend': 'torch'})
    m.set_X(coeffs, m.times)
    assert torch.equal(got, ref)
    paths = got[-1].reshape(B, Sn, H)
    assert torch.equal(got[0].reshape(B, Sn, H)[:, 0], got[0].reshape(B, Sn, H)[:, 2])      # one initial state per input row
    assert (paths[:, 0] - paths[:, 1]).abs().max() > 1e-3 and (paths[:, 1] - paths[:, 2]).abs().max() > 1e-3
    # y0 given per path, a row_out per input row, samples = 1
    again = S.sdeint(m, y0.repeat_interleave(Sn, 0), ts, dt=0.5, method=method, options={'samples': Sn, 'seed': 11, 'backend': 'torch'})
    assert torch.equal(again, got)
    one = S.sdeint(m, y0, ts, dt=0.5, method=method, options={'samples': 1, 'seed': 11, 'backend': 'torch'})
    assert torch.equal(one, S.sdeint(m, y0, ts, dt=0.5, method=method, options={'seed': 11, 'backend': 'torch'}))


def test_wrapper_returns_one_readout_row_per_path():
    m, pr = _model()
    net = S.NeuralSDE(m, pr['C'], pr['H'], 2).eval().requires_grad_(False)
    coeffs = torch.from_numpy(pr['coeffs'])
    final_index = torch.tensor([5, 3, 5, 2])
    with torch.no_grad():
        out = net(torch.from_numpy(pr['times']), (coeffs,), final_index, options={'samples': 3, 'seed': 2})
    assert tuple(out.shape) == (3 * pr['B'], 2)
    assert (out[0] - out[1]).abs().max() > 0


# ---- C ABI ------------------------------------------------------------------------------------------------------------------

def _solve(model, batch, samples=0, kernel='auto', method=0, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method, s.samples = model, batch, KNOTS, STEPS, 2, method, samples
    s.kernel = _lib.KERNELS[kernel]
    if method == 2:
        s.srk_tab = C.c_void_p(4096)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _path(s):
    return _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(s))]


def _launch_rc(s, workspace_bytes=0):
    """snsde_solve_forward validates before it touches a buffer: dummy non-null pointers, an error code back (a descriptor that
    passes the validation stops at SNSDE_ERR_WORKSPACE; with workspace_bytes set a refused one reaches the route)."""
    s.workspace_bytes = workspace_bytes
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(s, f, C.c_void_p(4096))
    return _lib.lib().snsde_solve_forward(C.byref(s), None)


def test_the_struct_grew_by_two_int32_and_the_abi_check_passes():
    lib = _lib.lib()
    names = [f[0] for f in _lib.Solve._fields_]
    assert names[-3:] == ['global_rows', 'samples', 'reserved3']
    assert lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve) - 8, 0, 0) != 0      # the struct before this field
    assert 'snsde_sample_stats' in _lib.EXPORTS and hasattr(lib, 'snsde_sample_stats')


def test_malformed_sample_counts_are_dimension_errors():
    model = elementwise_model(64)
    assert _launch_rc(_solve(model, 12, 3)) != ERR_DIMS                      # (a valid descriptor gets past the validation)
    assert _launch_rc(_solve(model, 12, 3, reserved3=1)) == ERR_DIMS
    assert _launch_rc(_solve(model, 12, 0, reserved3=1)) == ERR_DIMS
    assert _launch_rc(_solve(model, 13, 3)) == ERR_DIMS                      # batch % S
    assert _launch_rc(_solve(model, 12, 3, row_offset=4)) == ERR_DIMS        # row_offset % S
    assert _launch_rc(_solve(model, 12, 3, row_offset=6)) != ERR_DIMS
    assert _launch_rc(_solve(model, 12, -2)) == ERR_DIMS
    assert _launch_rc(_solve(model, 12, 3, global_rows=20)) == ERR_DIMS      # global_rows % S
    assert _launch_rc(_solve(model, 12, 3, global_rows=21)) != ERR_DIMS
    for bad in (_solve(model, 13, 3), _solve(model, 12, 3, row_offset=4), _solve(model, 12, 3, reserved3=1), _solve(model, 12, -2)):
        assert _path(bad) == 'none'


def test_sampled_solves_are_inference_only_in_the_library():
    lib = _lib.lib()
    model = elementwise_model(64)
    for f in ('act_save', 'stage_save', 'traj', 'dW_out', 'dU_out', 'z0_weight'):
        kw = {f: C.c_void_p(4096)}
        if f == 'z0_weight':
            kw['z0_bias'] = C.c_void_p(4096)
        assert _launch_rc(_solve(model, 12, 3, **kw)) == ERR_UNSUPPORTED, f
        assert _path(_solve(model, 12, 3, **kw)) == 'none', f
    for kernel in ('auto', 'generic', 'mfma4', 'mfma16'):
        for method in (0, 1, 2):
            s = _solve(model, 12, 3, kernel, method, traj=C.c_void_p(4096), dW_out=C.c_void_p(4096), act_save=C.c_void_p(4096))
            assert lib.snsde_backward_supported(C.byref(s)) == 0
            s = _solve(model, 12, 3, kernel, method)
            assert lib.snsde_backward_supported(C.byref(s)) == 0
            assert lib.snsde_backward_supported(C.byref(_solve(model, 12, 0, kernel, method))) != 0
    # the vector-field probe is per input row: refused as well (and taken without the field)
    p = C.c_void_p(4096)
    for samples, want in ((3, (ERR_UNSUPPORTED,)), (0, (-5,))):      # (-5: past the validation, at the workspace size)
        s = _solve(model, 12, samples, params=p, coeffs=p, workspace=p)
        assert lib.snsde_eval_fg(C.byref(s), p, p, p, p, None) in want
    b = _lib.Backward()
    b.fwd = _solve(model, 12, 3)
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(b.fwd, f, C.c_void_p(4096))
    b.grad_ys = b.adj = b.workspace = C.c_void_p(4096)
    assert lib.snsde_solve_backward(C.byref(b), None) == ERR_UNSUPPORTED
    b.fwd.traj = b.fwd.act_save = b.fwd.dW_out = b.delta_save = C.c_void_p(4096)      # (what a training forward would have left)
    assert lib.snsde_solve_backward(C.byref(b), None) == ERR_UNSUPPORTED
    assert lib.snsde_backward_with_gradients(C.byref(b), C.c_void_p(4096), C.c_void_p(4096), 1 << 20, None) == ERR_UNSUPPORTED
    assert lib.snsde_param_gradients(C.byref(b), C.c_void_p(4096), C.c_void_p(4096), 1 << 20, None) == ERR_UNSUPPORTED


def test_zero_and_one_sample_change_no_answer_of_the_route_fixture():
    """samples = 0 and samples = 1: every host query of every descriptor of tests/golden/routes.npz (the shapes
    tests/test_host_cpu.py plans) answers as before; samples = 4 never changes the workspace size."""
    g = load('routes.npz')
    assert tuple(g['fields']) == FIELDS
    lib = _lib.lib()
    wb = ANSWERS.index('workspace_bytes')
    n = 0
    for row, want in zip(g['desc'][::3], g['answers'][::3]):
        base = answers(row)
        assert base[0] == int(want[0]) and base[wb] == int(want[wb])      # (the recorded path and workspace; test_routes_cpu.py: the rest)
        for samples in (0, 1):
            s = solve_struct(row)
            s.samples = samples
            b = _lib.Backward()
            b.fwd = s
            assert [lib.snsde_forward_path(C.byref(s)), lib.snsde_backward_supported(C.byref(s)), lib.snsde_workspace_bytes(C.byref(s)),
                    lib.snsde_backward_workspace_bytes(C.byref(b))] == base[:4], (row, samples)
        d = dict(zip(FIELDS, (int(v) for v in row)))
        if d['batch'] % 4 == 0:
            s = solve_struct(row)
            s.samples = 4
            assert lib.snsde_workspace_bytes(C.byref(s)) == base[wb], row
            n += 1
    assert n > 200


def test_covered_families_plan_and_the_others_are_no_kernel():
    lean = elementwise_model(64)
    assert _path(_solve(lean, 12, 3)) == _path(_solve(lean, 12, 0)) == 'lean'
    assert _path(_solve(lean, 12, 3, 'mfma4')) == 'lean'
    assert _path(_solve(lean, 12, 3, flags=_lib.FLAG_BF16_OPERANDS)) == 'lean-bf16'
    assert _path(_solve(lean, 35, 7, 'mfma16')) == 'mfma16'
    assert _path(_solve(lean, 12, 3, 'mfma4', 2)) == 'mfma-srk' and _path(_solve(lean, 35, 7, 'mfma16', 2)) == 'mfma-srk'
    assert _path(_solve(lean, 12, 3, 'generic')) == 'generic' and _path(_solve(lean, 12, 3, 'generic', 2)) == 'generic-srk'
    wide = engine.model_struct(3, 48, 48, 2, 4, 17)            # no MFMA instantiation: `auto` arrives at the generic family
    assert _path(_solve(wide, 12, 3)) == _path(_solve(wide, 12, 0)) == 'generic'
    # families left uncovered: the wave pairs, the diffusion-net kernels, the streamed H = 256 lean kernels - no kernel at all,
    # not the generic family in their place
    net = net_model()
    assert _path(_solve(net, 12, 0)) == 'w4' and _path(_solve(net, 12, 3)) == 'none'
    assert _path(_solve(net, 12, 0, 'w4')) == 'w4' and _path(_solve(net, 12, 3, 'w4')) == 'none'
    assert _path(_solve(net, 12, 0, method=2)) != 'none' and _path(_solve(net, 12, 3, method=2)) == 'none'
    h256 = elementwise_model(256)
    assert _path(_solve(h256, 12, 0)) == 'lean-streamed' and _path(_solve(h256, 12, 3)) == 'none'
    assert _launch_rc(_solve(net, 12, 3), 1 << 30) == ERR_UNSUPPORTED and _launch_rc(_solve(h256, 12, 3), 1 << 30) == ERR_UNSUPPORTED
    # the Python query, and the workspace of a refused plan
    assert engine.forward_path(net, 12, KNOTS, STEPS, samples=3) == 'none'
    assert engine.forward_path(lean, 12, KNOTS, STEPS, samples=3) == 'lean'
    lib = _lib.lib()
    for model in (lean, net, h256, wide):
        assert lib.snsde_workspace_bytes(C.byref(_solve(model, 12, 3))) == lib.snsde_workspace_bytes(C.byref(_solve(model, 12, 0))) > 0


def test_stats_entry_point_validates_before_it_launches():
    lib = _lib.lib()
    p = C.c_void_p(4096)
    assert lib.snsde_sample_stats(None, 1, 2, 1, p, p, None) == -1 and lib.snsde_sample_stats(p, 1, 2, 1, None, p, None) == -1
    assert lib.snsde_sample_stats(p, 0, 2, 1, p, p, None) == ERR_DIMS
    assert lib.snsde_sample_stats(p, 1, 0, 1, p, None, None) == ERR_DIMS
    assert lib.snsde_sample_stats(p, 1, 2, 0, p, p, None) == ERR_DIMS
    assert lib.snsde_sample_stats(p, 1, 1, 4, p, p, None) == ERR_DIMS      # the unbiased variance of one sample


@pytest.mark.parametrize('shape, Sn', [((1, 2, 1), 2), ((5, 7 * 3, 33), 3), ((2, 3, 8 * 8, 16), 8)])
def test_sample_stats_on_cpu_tensors_match_float64(shape, Sn):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
    mean, var = S.sample_stats(torch.from_numpy(x), Sn)
    v = x.astype(np.float64).reshape(shape[:-2] + (shape[-2] // Sn, Sn, shape[-1]))
    assert tuple(mean.shape) == tuple(var.shape) == shape[:-2] + (shape[-2] // Sn, shape[-1])
    np.testing.assert_allclose(mean.numpy(), v.mean(-2), rtol=0, atol=(Sn + 1) * 2.0 ** -24 * np.abs(v).sum(-2).max() / Sn)
    np.testing.assert_allclose(var.numpy(), v.var(-2, ddof=1), rtol=1e-5, atol=1e-6)
    m2, none = S.sample_stats(torch.from_numpy(x), Sn, var=False)
    assert none is None and torch.equal(m2, mean)
    with pytest.raises(ValueError):
        S.sample_stats(torch.from_numpy(x), 5)
    with pytest.raises(ValueError):
        S.sample_stats(torch.from_numpy(x), 1)
