"""Model ensembles on the host: snsde_solve::members in the C struct and its host-only queries, what is refused and with which
code, the workspace of M prepared blocks, and sdeint_ensemble / Ensemble on CPU tensors against the loop of ordinary calls.
No GPU compute."""
import ctypes as C

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model, flip_batch, net_model
from tests.helpers import make_problem

ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4, -5
P = C.c_void_p(4096)


def _solve(model, batch, members=0, kernel='auto', method=0, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method, s.members = model, batch, KNOTS, STEPS, 2, method, members
    s.kernel = _lib.KERNELS[kernel]
    if method == 2:
        s.srk_tab = P
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _path(s):
    return _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(s))]


def _kernel(s):
    return engine.forward_kernel(s)


def _ws(s):
    return int(_lib.lib().snsde_workspace_bytes(C.byref(s)))


def _launch_rc(s, workspace_bytes=0):
    """snsde_solve_forward validates before it touches a buffer: dummy non-null pointers, an error code back (a descriptor that
    passes the validation stops at SNSDE_ERR_WORKSPACE; with workspace_bytes set a refused one reaches the route)."""
    s.workspace_bytes = workspace_bytes
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(s, f, P)
    return _lib.lib().snsde_solve_forward(C.byref(s), None)


def test_the_struct_keeps_its_size_and_the_reserved_slot_is_members():
    lib = _lib.lib()
    names = [f[0] for f in _lib.Solve._fields_]
    assert C.sizeof(_lib.Solve) == 304
    assert names[-3:] == ['global_rows', 'samples', 'reserved3']
    assert names[names.index('flags') + 1] == 'members' and 'reserved' not in names
    assert _lib.Solve.members.offset == _lib.Solve.flags.offset + 4 and _lib.Solve.members.size == 4
    assert lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0


@pytest.mark.parametrize('members', [0, 1])
def test_zero_and_one_member_answer_as_before(members):
    """members = 0 / 1 is one model: path, exact kernel and workspace of a handful of descriptors - lean, general, SRK, wave pairs,
    H = 256, the generic family, 16-row tiles - are those of the descriptor without the field."""
    lib = _lib.lib()
    wide = engine.model_struct(3, 48, 48, 2, 4, 17)
    cases = [(elementwise_model(64), 24, 'auto', 0), (elementwise_model(128), 24, 'mfma4', 1), (elementwise_model(128), 24, 'mfma4', 2),
             (net_model(), 24, 'auto', 0), (elementwise_model(256), 24, 'auto', 0), (wide, 24, 'auto', 0),
             (elementwise_model(128), 13, 'generic', 0), (elementwise_model(64), flip_batch(64), 'auto', 0)]
    for model, batch, kernel, method in cases:
        base, s = _solve(model, batch, 0, kernel, method), _solve(model, batch, members, kernel, method)
        base.members = 0
        assert _path(s) == _path(base) != 'none'
        assert _kernel(s) == _kernel(base)
        assert _ws(s) == _ws(base) > 0
        assert lib.snsde_backward_supported(C.byref(s)) == lib.snsde_backward_supported(C.byref(base))
        assert _launch_rc(s) == _launch_rc(base) == ERR_WORKSPACE      # (past the validation, as before)


def test_malformed_member_counts_are_dimension_errors():
    model = elementwise_model(64)
    assert _launch_rc(_solve(model, 24, 3)) == ERR_WORKSPACE               # (a valid descriptor gets past the validation)
    assert _launch_rc(_solve(model, 24, -1)) == ERR_DIMS
    assert _launch_rc(_solve(model, 13, 3)) == ERR_DIMS                    # batch % M
    assert _launch_rc(_solve(model, 18, 3)) == ERR_DIMS                    # Bm = 6: a tile would straddle two members
    for bad in (_solve(model, 24, -1), _solve(model, 13, 3), _solve(model, 18, 3)):
        assert _path(bad) == 'none' and _kernel(bad) == 'none'
        assert _lib.lib().snsde_backward_supported(C.byref(bad)) == 0


def test_ensembles_are_inference_only_in_the_library():
    lib = _lib.lib()
    model = elementwise_model(64)
    table = engine.model_struct(3, 64, 64, 2, 4, 13)      # (a supplied noise_table goes with noise_option 12 / 13)
    refused = [dict(samples=2), dict(z0_weight=P, z0_bias=P), dict(kl_column1=3)] + \
              [{f: P} for f in ('act_save', 'stage_save', 'traj', 'dW_out', 'dU_out')]
    for kw in refused:
        assert _path(_solve(model, 24, 0, **kw)) != 'none' or 'kl_column1' in kw, kw      # (refused for the members, not by itself)
        s = _solve(model, 24, 3, **kw)
        assert _path(s) == 'none' and _kernel(s) == 'none', kw
        assert lib.snsde_backward_supported(C.byref(s)) == 0, kw
        assert _launch_rc(_solve(model, 24, 3, **kw), 1 << 30) == ERR_UNSUPPORTED, kw
    assert _path(_solve(table, 24, 0, noise_table=P)) != 'none' and _path(_solve(table, 24, 3)) != 'none'
    assert _path(_solve(table, 24, 3, noise_table=P)) == 'none'
    assert lib.snsde_backward_supported(C.byref(_solve(table, 24, 3, noise_table=P))) == 0
    assert _launch_rc(_solve(table, 24, 3, noise_table=P), 1 << 30) == ERR_UNSUPPORTED
    # no adjoint of any kind, whatever the kernel selector and the method
    for kernel in ('auto', 'generic', 'mfma4', 'mfma16'):
        for method in (0, 1, 2):
            assert lib.snsde_backward_supported(C.byref(_solve(model, 24, 3, kernel, method))) == 0
            assert engine.backward_kernel(_solve(model, 24, 3, kernel, method)) == 'none'
            assert lib.snsde_backward_supported(C.byref(_solve(model, 24, 0, kernel, method))) != 0
    # every backward entry point and the vector-field probe
    for members, want in ((3, ERR_UNSUPPORTED), (0, ERR_WORKSPACE)):
        s = _solve(model, 24, members, params=P, coeffs=P, workspace=P)
        assert lib.snsde_eval_fg(C.byref(s), P, P, P, P, None) == want
    b = _lib.Backward()
    b.fwd = _solve(model, 24, 3)
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(b.fwd, f, P)
    b.grad_ys = b.adj = b.workspace = P
    for planes in (False, True):
        if planes:      # (what a training forward would have left)
            b.fwd.traj = b.fwd.act_save = b.fwd.dW_out = b.delta_save = P
        assert lib.snsde_solve_backward(C.byref(b), None) == ERR_UNSUPPORTED
        assert lib.snsde_backward_with_gradients(C.byref(b), P, P, 1 << 20, None) == ERR_UNSUPPORTED
        assert lib.snsde_param_gradients(C.byref(b), P, P, 1 << 20, None) == ERR_UNSUPPORTED
        assert lib.snsde_coeff_gradients(C.byref(b), P, P, 1 << 20, None) == ERR_UNSUPPORTED
        assert lib.snsde_backward_workspace_bytes(C.byref(b)) >= 0 and lib.snsde_param_gradients_workspace_bytes(C.byref(b)) == 0
        assert lib.snsde_coeff_gradients_workspace_bytes(C.byref(b)) == 0


def test_covered_kernels_plan_and_the_others_are_no_kernel():
    lean64, lean128, lean32 = elementwise_model(64), elementwise_model(128), elementwise_model(32)
    G = _lib.FLAG_LEAN_GENERAL
    for model in (lean32, lean64, lean128):
        for method in (0, 1):
            s = _solve(model, 24, 3, method=method, flags=G)
            assert _path(s) == 'lean' and _kernel(s) == 'lean' and engine.lean_variant(s) == 'general'
    k2 = engine.model_struct(21, 128, 128, 2, 4, 17)      # (the compile-time specialised instantiation: H = 128, C = 21)
    assert engine.lean_variant(_solve(k2, 24, 3)) == engine.lean_variant(_solve(k2, 24, 0)) == 'specialised'
    assert engine.lean_variant(_solve(k2, 24, 3, flags=G)) == 'general'
    assert _kernel(_solve(lean128, 24, 3, flags=_lib.FLAG_BF16_OPERANDS)) == 'lean_bf16'
    assert _kernel(_solve(lean64, 24, 3, flags=_lib.FLAG_BF16_OPERANDS)) == 'lean_bf16'
    # the general kernel under Euler: a diffusion net at H = 64 when 4-row tiles are asked for by name, and the unfused emb order
    assert _kernel(_solve(net_model(), 24, 0, 'mfma4')) == _kernel(_solve(net_model(), 24, 3, 'mfma4')) == 'general_m4'
    assert _kernel(_solve(lean128, 24, 3, 'mfma4', flags=_lib.FLAG_EXACT_ORDER)) == 'general_m4'
    assert _path(_solve(lean128, 24, 3, 'mfma4', 2)) == 'mfma-srk' and _kernel(_solve(lean128, 24, 3, 'mfma4', 2)) == 'general_m4'
    assert _kernel(_solve(lean128, 24, 3, 'auto', 2)) == 'general_m4'
    # plans that arrive at another kernel: no kernel at all, never the generic family in their place
    net, h256 = net_model(), elementwise_model(256)
    assert _path(_solve(net, 24, 0)) == 'w4' and _path(_solve(net, 24, 3)) == 'none'                    # wave pairs
    assert _path(_solve(net, 24, 0, 'w4')) == 'w4' and _path(_solve(net, 24, 3, 'w4')) == 'none'
    assert _kernel(_solve(net, 24, 0, method=2)) == 'w4' and _path(_solve(net, 24, 3, method=2)) == 'none'
    net128 = engine.model_struct(3, 128, 128, 2, 1, 18)
    assert _kernel(_solve(net128, 24, 0)) == 'm4n' and _path(_solve(net128, 24, 3)) == 'none'      # diffusion-net kernel
    assert _path(_solve(h256, 24, 0)) == 'lean-streamed' and _path(_solve(h256, 24, 3)) == 'none'      # H = 256
    assert _kernel(_solve(lean64, 48, 0, 'mfma16')) == 'general_m16' and _path(_solve(lean64, 48, 3, 'mfma16')) == 'none'   # 16-row tiles
    big = 3 * flip_batch(64)      # `auto` leaves the 4-row tiles: no plan either
    assert _kernel(_solve(lean64, big, 0)) == 'general_m16' and _path(_solve(lean64, big, 3)) == 'none'
    assert _kernel(_solve(lean128, 24, 0, flags=_lib.FLAG_TWO_TILE)) == 'lean_two_tile_h128'
    assert _path(_solve(lean128, 24, 3, flags=_lib.FLAG_TWO_TILE)) == 'none'                            # the two-tile kernels
    wide = engine.model_struct(3, 48, 48, 2, 4, 17)      # no MFMA instantiation: one model takes the generic family, an ensemble nothing
    assert _path(_solve(wide, 24, 0)) == 'generic' and _path(_solve(wide, 24, 3)) == 'none'
    assert _path(_solve(lean64, 24, 0, 'generic')) == 'generic' and _path(_solve(lean64, 24, 3, 'generic')) == 'none'
    for s in (_solve(net, 24, 3), _solve(h256, 24, 3), _solve(wide, 24, 3), _solve(lean64, 24, 3, 'generic')):
        assert _launch_rc(s, 1 << 30) == ERR_UNSUPPORTED
    # the Python queries
    assert engine.forward_path(net, 24, KNOTS, STEPS, members=3) == 'none'
    assert engine.forward_path(lean64, 24, KNOTS, STEPS, members=3) == 'lean'
    assert engine.forward_kernel(engine.query_descriptor(lean128, 24, KNOTS, STEPS, 'srk', members=3)) == 'general_m4'


def test_the_workspace_is_one_block_per_member():
    """snsde_workspace_bytes = M x the per-member block; the block is a whole number of 16-byte units (every member's f32x4 loads
    stay aligned), is no larger than one model's workspace, and does not depend on M."""
    for model, method in ((elementwise_model(64), 0), (elementwise_model(128), 0), (elementwise_model(128), 2), (elementwise_model(32), 1)):
        one = _ws(_solve(model, 48, 0, method=method))
        blocks = {}
        for M in (2, 3, 4, 6):
            total = _ws(_solve(model, 48, M, method=method))
            assert total % M == 0
            blocks[M] = total // M
        block = blocks[2]
        assert all(b == block for b in blocks.values()), blocks
        # (one model's query also covers the generic family's layout, which no ensemble launch uses: the block is never larger)
        assert block % 16 == 0 and 0 < block <= one + 12, (block, one)
        # a launch with less is refused, with exactly that much it is past the size check (no device here: the launch itself fails later)
        assert _launch_rc(_solve(model, 48, 3, method=method), 3 * block - 1) == ERR_WORKSPACE
    # no MFMA plan, no ensemble launch: the query answers as for one model
    wide = engine.model_struct(3, 48, 48, 2, 4, 17)
    assert _ws(_solve(wide, 24, 3)) == _ws(_solve(wide, 24, 0)) > 0


def test_initial_state_entry_point_validates_before_it_launches():
    lib = _lib.lib()
    assert 'snsde_initial_state' in _lib.EXPORTS and hasattr(lib, 'snsde_initial_state')
    s = _solve(elementwise_model(64), 24)
    assert lib.snsde_initial_state(None, None) == ERR_NULL
    assert lib.snsde_initial_state(C.byref(s), None) == ERR_NULL           # no coeffs
    s.coeffs = s.step_tab = s.y0 = P
    assert lib.snsde_initial_state(C.byref(s), None) == ERR_NULL           # no z0_weight / z0_bias
    s.z0_weight = s.z0_bias = P
    s.batch = 0
    assert lib.snsde_initial_state(C.byref(s), None) == ERR_DIMS
    s.batch, s.struct_size = 24, 8
    assert lib.snsde_initial_state(C.byref(s), None) == -10


# ---- sdeint_ensemble / Ensemble on CPU tensors --------------------------------------------------------------------------------

TIMES = np.array([0., 0.7, 1.9, 2.4, 4.1, 5.], np.float32)


def _members(M=3, B=4, H=16, C_=3, L=6, io=4, no=17, arch=None):
    """M modules of one architecture with different random parameters on one control path; arch: (H, num_hidden_layers) of
    the last member where it is to differ."""
    pr = make_problem(5, io, no, 2, B, H, C_, L, times=TIMES[:L])
    coeffs, times = torch.from_numpy(pr['coeffs']), torch.from_numpy(pr['times'])
    sdes = []
    for m in range(M):
        h, nl = arch if (arch and m == M - 1) else (H, 2)
        torch.manual_seed(100 + m)
        sde = S.Diffusion_model(C_, h, h, nl, input_option=io, noise_option=no).requires_grad_(False)
        sde.set_X(coeffs, times)
        sdes.append(sde)
    y0 = torch.from_numpy(np.random.default_rng(9).standard_normal((M, B, H)).astype(np.float32) * 0.5)
    return sdes, y0, times


def _loop(sdes, y0, ts, method, dt, options, global_rows=None):
    M, B = y0.shape[:2]
    off = options.get('row_offset', 0)
    outs = [S.sdeint(sde, y0[m], ts, method=method, dt=dt,
                     options=dict(options, row_offset=off + m * B, global_rows=global_rows or M * B)) for m, sde in enumerate(sdes)]
    return torch.stack(outs, dim=0 if 'row_out' in options else 1)


@pytest.mark.parametrize('method', ['euler', 'milstein', 'srk'])
@pytest.mark.parametrize('backend', ['auto', 'torch'])
def test_cpu_ensemble_equals_the_loop_of_ordinary_solves(method, backend):
    sdes, y0, times = _members()
    ts = torch.tensor([0., 1.3, 2.2, 5.])
    opts = {'seed': 11, 'backend': backend}
    got = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=opts)
    assert tuple(got.shape) == (4, 3, 4, 16)
    assert torch.equal(got, _loop(sdes, y0, ts, method, 0.5, opts))
    assert (got[-1, 0] - got[-1, 1]).abs().max() > 1e-3      # different members, different solutions
    # a row_out of length B selects per row inside every member; row_offset / global_rows are handed down
    ro = {'seed': 11, 'backend': backend, 'row_out': torch.tensor([3, 1, 0, 2]), 'row_offset': 8, 'global_rows': 64}
    sel = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=ro)
    assert tuple(sel.shape) == (3, 4, 16)
    assert torch.equal(sel, _loop(sdes, y0, ts, method, 0.5, ro, global_rows=64))
    assert torch.equal(sel[:, 0], got[3][:, 0]) or backend == 'auto'      # (the torch backend has no row stream: offsets move nothing)


def test_cpu_ensemble_of_different_architectures_loops_and_strict_raises():
    sdes, y0, times = _members(arch=(16, 3))
    ts = torch.tensor([0., 2.2, 5.])
    got = S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'seed': 3})
    assert torch.equal(got, _loop(sdes, y0, ts, 'euler', 0.5, {'seed': 3}))
    for strict_case in (sdes, _members()[0]):      # an uncovered plan - here: CPU tensors have no fused solve at all
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(strict_case, y0, ts, method='euler', dt=0.5, options={'seed': 3, 'strict': True})


def test_ensemble_is_inference_only():
    sdes, y0, times = _members()
    ts = torch.tensor([0., 2.2, 5.])
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, y0.clone().requires_grad_(True), ts, method='euler', dt=0.5)
    sdes[1].requires_grad_(True)
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5)
    with torch.no_grad():      # (no autograd: accepted)
        assert S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'seed': 1}).shape == (3, 3, 4, 16)
    sdes[1].requires_grad_(False)
    coeffs = sdes[0].coeffs.clone().requires_grad_(True)
    for sde in sdes:
        sde.set_X(coeffs, sde.times)
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5)
    for sde in sdes:
        sde.set_X(coeffs.detach(), sde.times)
    with pytest.raises(ValueError, match='samples'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'samples': 2})
    for opt in ({'save_traj': True}, {'recompute': 2}, {'z0_linear': torch.nn.Linear(3, 16)}):
        with pytest.raises(ValueError, match='inference only'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options=opt)
    with pytest.raises(ValueError, match='members, batch, channels'):
        S.sdeint_ensemble(sdes, y0[0], ts, method='euler', dt=0.5)
    with pytest.raises(ValueError, match='members, batch, channels'):
        S.sdeint_ensemble(sdes[:2], y0, ts, method='euler', dt=0.5)
    with pytest.raises(ValueError, match='row_out'):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'row_out': torch.zeros(12, dtype=torch.int64)})


def _wrappers(kind, M=3, B=4, H=16, C_=3, L=6):
    pr = make_problem(5, 4, 17, 2, B, H, C_, L, times=TIMES[:L])
    models = []
    for m in range(M):
        torch.manual_seed(40 + m)
        func = S.Diffusion_model(C_, H, H, 2, input_option=4, noise_option=17)
        net = kind(func, C_, 2, H, 3) if kind is S.NeuralSDE_forecasting else kind(func, C_, H, 3)
        models.append(net.eval().requires_grad_(False))
    return models, torch.from_numpy(pr['coeffs']), torch.from_numpy(pr['times'])


@pytest.mark.parametrize('kind', [S.NeuralSDE, S.NeuralSDE_forecasting, S.IstsNeuralSDE])
def test_cpu_ensemble_module_equals_the_wrappers_one_after_the_other(kind):
    models, coeffs, times = _wrappers(kind)
    M, B = len(models), coeffs.shape[0]
    ens = S.Ensemble(models).eval()
    fi = torch.tensor([5, 3, 5, 2])
    args = (coeffs, times) if kind is S.IstsNeuralSDE else (times, (coeffs,), fi)
    with torch.no_grad():
        got = ens(*args, options={'seed': 7})
        refs = [net(*args, options={'seed': 7, 'row_offset': m * B, 'global_rows': M * B}) for m, net in enumerate(models)]
    if kind is S.IstsNeuralSDE:
        assert tuple(got[0].shape) == (M,) + tuple(refs[0][0].shape) and tuple(got[1].shape) == (M,) + tuple(refs[0][1].shape)
        assert torch.equal(got[0], torch.stack([r[0] for r in refs])) and torch.equal(got[1], torch.stack([r[1] for r in refs]))
    else:
        assert tuple(got.shape) == (M,) + tuple(refs[0].shape)
        assert torch.equal(got, torch.stack(refs))
    with pytest.raises(ValueError, match='ONE class'):
        S.Ensemble(models + [torch.nn.Linear(2, 2)])
    with pytest.raises(ValueError, match='inference only'):
        ens.requires_grad_(True)(*args, options={'seed': 7})
