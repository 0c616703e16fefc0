"""Model ensembles on the wave-pair and diffusion-net kernels on the host (SNSDE_FLAG_ENSEMBLE_NETS, options={'ensemble_nets':
True}): the flag in the C ABI and its host-only queries - what it opens (members = M > 1 on FwdKernel::w4 / FwdKernel::m4n, with
SNSDE_FLAG_ENSEMBLE_SAMPLES their sample paths), what it leaves refused (z0_weight, noise_table, kl_column1, bf16 operands, the
generic family, every training plane), the dimension errors, the workspace of M member-alone blocks - and sdeint_ensemble on CPU
tensors.  No GPU compute."""
import ctypes as C
import os
import re

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, net_model
from tests.test_ensemble_cpu import _members

ERR_NULL, ERR_DIMS, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4, -5
P = C.c_void_p(4096)
EN, ES, EG, SG = 1024, 512, 256, 64
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'snsde.h')


def net128():
    """H = 128, latent-only drift, two-layer diffusion net: snsde_m4n_kernel under every method."""
    return engine.model_struct(3, 128, 128, 2, 1, 18)


def net_control():
    """H = 64, embedded drift on a control path, two-layer diffusion net times y: snsde_m4n_kernel under Milstein and SRK (Milstein
    at H = 128 has no instantiation)."""
    return engine.model_struct(3, 64, 64, 2, 4, 19)


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


def _ws(s):
    return int(_lib.lib().snsde_workspace_bytes(C.byref(s)))


def _launch_rc(s, workspace_bytes=0):
    """snsde_solve_forward validates before it touches a buffer: dummy non-null pointers, an error code back."""
    s.workspace_bytes = workspace_bytes
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(s, f, P)
    return _lib.lib().snsde_solve_forward(C.byref(s), None)


def _answers(s):
    lib = _lib.lib()
    b = _lib.Backward()
    b.fwd = s
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(b.fwd, f, P)
    b.grad_ys = b.adj = b.workspace = b.delta_save = P
    return (_path(s), engine.forward_kernel(s), engine.backward_kernel(s), _ws(s), int(lib.snsde_backward_supported(C.byref(s))),
            int(lib.snsde_backward_workspace_bytes(C.byref(b))), int(lib.snsde_param_gradients_workspace_bytes(C.byref(b))))


# the descriptors of the issue: (model, kernel selector, method) -> (path, kernel) under the flag
W4_CASES = [('auto', 0), ('w4', 0), ('auto', 2), ('w4', 2)]
M4N_CASES = [('auto', 0, 'mfma4'), ('mfma4', 0, 'mfma4'), ('auto', 2, 'mfma-srk'), ('mfma4', 2, 'mfma-srk')]


def test_flag_value_struct_size_and_version():
    lib = _lib.lib()
    assert _lib.FLAG_ENSEMBLE_NETS == EN == 1024
    assert C.sizeof(_lib.Solve) == 304 and C.sizeof(_lib.Backward) == 368 and lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0
    assert re.search(r'SNSDE_FLAG_ENSEMBLE_NETS\s*=\s*1024', open(HEADER).read())


@pytest.mark.parametrize('members', [0, 1])
def test_the_flag_alone_changes_nothing(members):
    """members <= 1: path, kernel, workspaces and every backward answer are those without the flag, for inference and training
    descriptors, with and without sample paths."""
    for model in (net_model(), net128()):
        for kernel, method in (('auto', 0), ('mfma4', 1), ('mfma4', 2), ('auto', 2)):
            for samples, extra in ((0, 0), (2, 0), (2, ES), (2, SG)):
                for train in (False, True):
                    base = _solve(model, 24, members, samples, kernel, method, flags=extra)
                    flag = _solve(model, 24, members, samples, kernel, method, flags=extra | EN)
                    if train:
                        _train(base), _train(flag)
                    assert _answers(flag) == _answers(base), (members, samples, kernel, method, train, extra)


def test_the_flag_opens_the_wave_pairs_and_the_diffusion_net_tiles():
    lib = _lib.lib()
    for kernel, method in W4_CASES:
        on, off = _solve(net_model(), 24, 3, 0, kernel, method, flags=EN), _solve(net_model(), 24, 3, 0, kernel, method)
        assert _path(off) == 'none' and engine.forward_kernel(off) == 'none', (kernel, method)
        assert _path(on) == 'w4' and engine.forward_kernel(on) == 'w4', (kernel, method)
        assert engine.forward_kernel(off, ensemble_nets=True) == 'w4' and off.flags == 0      # (a copy carries the flag)
        # the member alone as a shard of the whole runs the same kernel
        assert engine.forward_kernel(_solve(net_model(), 8, 0, 0, kernel, method, row_offset=8, global_rows=24)) == 'w4'
        assert lib.snsde_backward_supported(C.byref(on)) == 0 and engine.backward_kernel(on) == 'none'
    for kernel, method, path in M4N_CASES:
        on, off = _solve(net128(), 24, 3, 0, kernel, method, flags=EN), _solve(net128(), 24, 3, 0, kernel, method)
        assert _path(off) == 'none' and engine.forward_kernel(off) == 'none', (kernel, method)
        assert _path(on) == path and engine.forward_kernel(on) == 'm4n', (kernel, method)
        assert engine.forward_kernel(_solve(net128(), 8, 0, 0, kernel, method, row_offset=8, global_rows=24)) == 'm4n'
        assert lib.snsde_backward_supported(C.byref(on)) == 0 and engine.backward_kernel(on) == 'none'
    # the other hidden sizes of snsde_m4n_kernel, the embedded drift with a control path, Milstein's transposed layers
    for H in (16, 32, 64):
        assert engine.forward_kernel(_solve(engine.model_struct(3, H, H, 2, 3, 18), 24, 3, 0, 'mfma4', 2, flags=EN)) == 'm4n'
    assert engine.forward_kernel(_solve(engine.model_struct(3, 32, 32, 2, 4, 18), 24, 3, 0, 'auto', 2, flags=EN)) == 'm4n'
    assert engine.forward_kernel(_solve(net_control(), 24, 3, 0, 'auto', 1, flags=EN)) == 'm4n'
    assert engine.forward_kernel(_solve(engine.model_struct(40, 64, 64, 2, 4, 18), 24, 3, 0, 'auto', 0, flags=EN)) == 'm4n'
    # the Python queries
    q = dict(members=3, global_rows=24)
    assert engine.forward_path(net_model(), 24, KNOTS, STEPS, ensemble_nets=True, **q) == 'w4'
    assert engine.forward_path(net_model(), 24, KNOTS, STEPS, 'srk', ensemble_nets=True, **q) == 'w4'
    assert engine.forward_path(net_model(), 24, KNOTS, STEPS, **q) == 'none'
    assert engine.forward_path(net128(), 24, KNOTS, STEPS, 'srk', ensemble_nets=True, **q) == 'mfma-srk'
    assert engine.forward_kernel(engine.query_descriptor(net128(), 24, KNOTS, STEPS, 'srk', ensemble_nets=True, **q)) == 'm4n'
    assert engine.forward_kernel(engine.query_descriptor(net128(), 24, KNOTS, STEPS, 'srk', **q)) == 'none'
    # what the flag does not concern keeps its answer: the kernels that take members without it
    lean = engine.model_struct(3, 64, 64, 2, 4, 17)
    assert _answers(_solve(lean, 24, 3, flags=EN)) == _answers(_solve(lean, 24, 3))


def test_sample_paths_of_the_ensemble_need_both_flags():
    for model, kernel, method, fwd in ((net_model(), 'auto', 0, 'w4'), (net_model(), 'auto', 2, 'w4'), (net128(), 'auto', 2, 'm4n'),
                                       (net_control(), 'mfma4', 1, 'm4n')):
        assert engine.forward_kernel(_solve(model, 24, 3, 2, kernel, method, flags=EN | ES)) == fwd
        assert _path(_solve(model, 24, 3, 2, kernel, method, flags=EN | ES)) != 'none'
        for flags in (EN, ES, 0):
            s = _solve(model, 24, 3, 2, kernel, method, flags=flags)
            assert _path(s) == 'none' and engine.forward_kernel(s) == 'none', (fwd, flags)
            assert _launch_rc(_solve(model, 24, 3, 2, kernel, method, flags=flags), 1 << 30) == ERR_UNSUPPORTED
        # plain samples on one model stay refused on these kernels, with or without the flags
        for flags in (0, EN, EN | ES):
            assert _answers(_solve(model, 24, 0, 2, kernel, method, flags=flags)) == _answers(_solve(model, 24, 0, 2, kernel, method))
            assert _path(_solve(model, 24, 0, 2, kernel, method, flags=flags)) == 'none'
        # whole groups of paths per member
        assert _launch_rc(_solve(model, 24, 3, 3, kernel, method, flags=EN | ES)) == ERR_DIMS      # Bm = 8, S = 3
        assert engine.forward_path(model, 24, KNOTS, STEPS, ('euler', 'milstein', 'srk')[method], kernel, members=3, samples=2,
                                   ensemble_samples=True, ensemble_nets=True) != 'none'


def test_still_refused_under_the_flag():
    lib = _lib.lib()
    for model, kernel, method in ((net_model(), 'auto', 0), (net_model(), 'auto', 2), (net128(), 'auto', 2), (net_control(), 'auto', 1)):
        assert _path(_solve(model, 24, 3, 0, kernel, method, flags=EN)) != 'none'
        refused = [dict(z0_weight=P, z0_bias=P), dict(kl_column1=3), dict(flags=EN | _lib.FLAG_BF16_OPERANDS), dict(kernel='generic'),
                   dict(kernel='mfma16')]
        for kw in refused:
            args = dict(dict(kernel=kernel, flags=EN), **kw)
            s = _solve(model, 96 if kw.get('kernel') == 'mfma16' else 24, 3, 0, method=method, **args)
            assert _path(s) == 'none' and engine.forward_kernel(s) == 'none', kw
            assert lib.snsde_backward_supported(C.byref(s)) == 0 and engine.backward_kernel(s) == 'none', kw
            assert _launch_rc(s, 1 << 30) == ERR_UNSUPPORTED, kw
        # dimension errors: batch % M, Bm % 4
        for batch in (25, 18):
            s = _solve(model, batch, 3, 0, kernel, method, flags=EN)
            assert _path(s) == 'none' and _launch_rc(s) == ERR_DIMS, batch
        # every training plane, with or without SNSDE_FLAG_ENSEMBLE_GRAD
        for flags in (EN, EN | EG):
            for plane in ('act_save', 'traj', 'dW_out', 'stage_save', 'dU_out'):
                s = _solve(model, 24, 3, 0, kernel, method, flags=flags, **{plane: P})
                assert _path(s) == 'none' and lib.snsde_backward_supported(C.byref(s)) == 0, (flags, plane)
                assert engine.backward_kernel(s) == 'none'
            s = _train(_solve(model, 24, 3, 0, kernel, method, flags=flags))
            assert _path(s) == 'none' and engine.forward_kernel(s) == 'none', flags
            assert lib.snsde_backward_supported(C.byref(s)) == 0 and engine.backward_kernel(s) == 'none'
            assert _launch_rc(s, 1 << 30) == ERR_UNSUPPORTED
    # a supplied noise_table goes with noise_option 12 / 13, which no net kernel runs: refused as for every ensemble
    table = engine.model_struct(3, 64, 64, 2, 4, 13)
    assert _path(_solve(table, 24, 3, flags=EN, noise_table=P)) == 'none'
    # the field variants of snsde_m4n_kernel
    variant = engine.model_struct(3, 64, 64, 2, 4, 18)
    variant.activation, variant.drift_output, variant.diffusion_output, variant.time_feature = 1, 1, 2, 1
    assert engine.forward_kernel(_solve(variant, 24, 0, 0, 'auto', 2)) == 'm4n'
    assert _path(_solve(variant, 24, 3, 0, 'auto', 2, flags=EN)) == 'none'
    grid = type('G', (), {'N': STEPS, 'T': 2})
    assert engine.backward_mode(net_model(), 24, KNOTS, grid, 'euler', members=3, ensemble_grad=True) == 0


def test_the_workspace_is_m_member_alone_blocks():
    """snsde_workspace_bytes = M x (the plan's floats rounded up to a multiple of four + the 64-float tail): per snsde.h the block of
    an ensemble is that of the member-alone plan, whose own query answers plan floats + 64 where no generic layout is larger."""
    for model, kernel, method in ((net_model(), 'auto', 0), (net_model(), 'auto', 2), (net128(), 'auto', 2), (net_control(), 'auto', 1),
                                  (engine.model_struct(40, 64, 64, 2, 4, 18), 'auto', 0)):
        blocks = {}
        for M in (2, 3, 6):
            total = _ws(_solve(model, 48, M, 0, kernel, method, flags=EN))
            assert total % M == 0
            blocks[M] = total // M
        block = blocks[3]
        assert all(b == block for b in blocks.values()) and block % 16 == 0 and block > 0
        assert _ws(_solve(model, 48, 3, 0, kernel, method)) == 3 * block      # (the query does not depend on the flag)
        one = _ws(_solve(model, 16, 0, 0, kernel, method, row_offset=16, global_rows=48))      # the member alone, as a shard
        assert 0 < block <= one + 12, (block, one)
        # a launch with no workspace, and with one byte less than the query's answer, is refused for its size
        assert _launch_rc(_solve(model, 48, 3, 0, kernel, method, flags=EN), 0) == ERR_WORKSPACE
        assert _launch_rc(_solve(model, 48, 3, 0, kernel, method, flags=EN), 3 * block - 1) == ERR_WORKSPACE


# ---- front end on CPU tensors ---------------------------------------------------------------------------------------------------

def test_option_checks():
    sdes, y0, times = _members(io=1, no=18)
    ts = torch.tensor([0., 2.2, 5.])
    for bad in (1, 'yes', None, 0):
        with pytest.raises(ValueError, match='ensemble_nets must be a bool'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets': bad})
        with pytest.raises(ValueError, match='ensemble_nets must be a bool'):
            engine.check_ensemble_nets(bad)
    assert engine.check_ensemble_nets(True) is True and engine.check_ensemble_nets(False) is False
    with pytest.raises(NotImplementedError, match='strict'):      # CPU tensors have no fused solve, with or without the option
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets': True, 'strict': True})
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, y0.clone().requires_grad_(True), ts, method='euler', dt=0.5, options={'ensemble_nets': True})


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_cpu_ensemble_with_the_option_equals_the_loop_of_members(method):
    sdes, y0, times = _members(io=1, no=18)      # M = 3, B = 4, H = 16
    M, B = 3, 4
    ts = torch.tensor([0., 1.3, 2.2, 5.])
    with torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options={'seed': 11, 'ensemble_nets': True})
        ref = torch.stack([S.sdeint(sde, y0[m], ts, method=method, dt=0.5,
                                    options={'seed': 11, 'row_offset': m * B, 'global_rows': M * B}) for m, sde in enumerate(sdes)], dim=1)
        assert tuple(got.shape) == (4, M, B, 16) and torch.equal(got, ref)
        assert torch.equal(got, S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options={'seed': 11, 'ensemble_nets': False}))
        assert (got[-1, 0] - got[-1, 1]).abs().max() > 1e-3
        # with sample paths as well
        Sn = 2
        opts = {'seed': 11, 'samples': Sn, 'ensemble_samples': True, 'ensemble_nets': True}
        gs = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=0.5, options=opts)
        rs = torch.stack([S.sdeint(sde, y0[m], ts, method=method, dt=0.5,
                                   options={'seed': 11, 'samples': Sn, 'row_offset': m * B * Sn, 'global_rows': M * B * Sn})
                          for m, sde in enumerate(sdes)], dim=1)
        assert tuple(gs.shape) == (4, M, B * Sn, 16) and torch.equal(gs, rs)


def test_cpu_ensemble_module_passes_the_option_through():
    from tests.test_ensemble_cpu import _wrappers
    models, coeffs, times = _wrappers(S.NeuralSDE)
    M, B = len(models), coeffs.shape[0]
    ens = S.Ensemble(models).eval()
    fi = torch.tensor([5, 3, 5, 2])
    with torch.no_grad():
        got = ens(times, (coeffs,), fi, options={'seed': 7, 'ensemble_nets': True})
        refs = [net(times, (coeffs,), fi, options={'seed': 7, 'row_offset': m * B, 'global_rows': M * B}) for m, net in enumerate(models)]
        assert torch.equal(got, torch.stack(refs))
        with pytest.raises(ValueError, match='ensemble_nets must be a bool'):
            ens(times, (coeffs,), fi, options={'seed': 7, 'ensemble_nets': 1})
