"""Training through wave-pair model ensembles on the host (SNSDE_FLAG_ENSEMBLE_NETS_GRAD, options={'ensemble_nets_grad': True}): the
flag in the C ABI and its host-only queries - what the three flags ENSEMBLE_NETS | ENSEMBLE_GRAD | ENSEMBLE_NETS_GRAD open together
(training planes on FwdKernel::w4, snsde_backward_supported == 1 on RevKernel::w4_fused, no delta planes, a backward workspace of M
member-alone blocks), that any two of them answer as before, what stays refused under all three - and sdeint_ensemble on CPU tensors.
No GPU compute."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS
from tests.test_ensemble_cpu import _members

P = C.c_void_p(4096)
ENG, EN, ES, EG, SG = 2048, 1024, 512, 256, 64
ALL = ENG | EN | EG
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'snsde.h')
M = 3


def _model(io=1, no=18, NL=2, H=64):
    return engine.model_struct(3, H, H, NL, io, no)


def _solve(model, batch, members=M, samples=0, kernel='auto', method=0, flags=ALL, train=True, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method = model, batch, KNOTS, STEPS, 2, method
    s.members, s.samples = members, samples
    s.kernel, s.flags = _lib.KERNELS[kernel], flags
    if method == 2:
        s.srk_tab = P
    if train:
        s.traj = s.act_save = s.dW_out = P
        if method == 2:
            s.stage_save = s.dU_out = P
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _backward(s):
    b = _lib.Backward()
    b.fwd = s
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(b.fwd, f, P)
    b.grad_ys = b.adj = b.workspace = P
    return b


def _answers(s):
    """(path, forward kernel, adjoint kernel, backward mode, forward / backward / parameter-pass workspace bytes)"""
    lib = _lib.lib()
    b = _backward(s)
    return (_lib.PATHS[lib.snsde_forward_path(C.byref(s))], engine.forward_kernel(s), engine.backward_kernel(s),
            int(lib.snsde_backward_supported(C.byref(s))), int(lib.snsde_workspace_bytes(C.byref(s))),
            int(lib.snsde_backward_workspace_bytes(C.byref(b))), int(lib.snsde_param_gradients_workspace_bytes(C.byref(b))))


def _refused(s, what):
    a = _answers(s)
    assert a[0] == 'none' and a[1] == 'none' and a[2] == 'none' and a[3] == 0, (what, a)


def test_flag_value_struct_size_and_version():
    lib = _lib.lib()
    assert _lib.FLAG_ENSEMBLE_NETS_GRAD == ENG == 2048
    assert C.sizeof(_lib.Solve) == 304 and lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0
    assert re.search(r'SNSDE_FLAG_ENSEMBLE_NETS_GRAD\s*=\s*2048', open(HEADER).read())


@pytest.mark.parametrize('method', [0, 2])
@pytest.mark.parametrize('NL', [1, 2])
@pytest.mark.parametrize('no', [14, 15, 18, 19])
@pytest.mark.parametrize('io', [1, 3, 5])
def test_the_three_flags_open_training_on_the_wave_pairs(io, no, NL, method):
    lib = _lib.lib()
    model = _model(io, no, NL)
    for Bm in (4, 8, 12):
        s = _solve(model, M * Bm, method=method)
        path, fwd, rev, mode, fws, bws, pws = _answers(s)
        assert (path, fwd, rev, mode) == ('w4', 'w4', 'w4_fused', 1), (Bm, path, fwd, rev, mode)
        slots, planes, dslots = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        assert lib.snsde_save_layout(C.byref(s), C.byref(slots), C.byref(planes), C.byref(dslots)) == 0
        assert dslots.value == 0 and slots.value > 0 and planes.value == (3 if method == 2 else 1)
        # the member alone, as a shard of the whole: the same kernels, and its block of the backward workspace
        one = _solve(model, Bm, members=0, method=method, flags=0, row_offset=Bm, global_rows=M * Bm)
        p1, f1, r1, m1, fws1, bws1, pws1 = _answers(one)
        assert (p1, f1, r1, m1) == ('w4', 'w4', 'w4_fused', 1)
        assert bws1 % 4 == 0 and bws == M * ((bws1 + 15) & ~15), (Bm, bws, bws1)      # (snsde_member_bws_stride: 16-byte blocks)
        assert pws == M * ((pws1 + 15) & ~15) and pws > 0
        # the forward workspace is the ensemble's: that of the inference descriptor under SNSDE_FLAG_ENSEMBLE_NETS
        assert fws == _answers(_solve(model, M * Bm, method=method, flags=EN, train=False))[4] and fws % M == 0 and fws > 0
        # drop any one of the three flags: the parent's answers
        for drop in (ENG, EN, EG):
            _refused(_solve(model, M * Bm, method=method, flags=ALL & ~drop), (Bm, drop))
        # the inference descriptor keeps its answers whatever the new flag says
        assert _answers(_solve(model, M * Bm, method=method, flags=EN | ENG, train=False)) == \
            _answers(_solve(model, M * Bm, method=method, flags=EN, train=False))


def test_alone_or_with_one_other_flag_it_changes_no_answer():
    """Every subset of the other flags, with and without SNSDE_FLAG_ENSEMBLE_NETS_GRAD: equal answers unless all three are set;
    one model (members <= 1): equal answers always."""
    lean = engine.model_struct(3, 64, 64, 2, 4, 17)
    for model, method, kernel in itertools.product((_model(), _model(1, 18, 2, 128), lean), (0, 1, 2), ('auto', 'mfma4', 'w4')):
        for members, samples, train in itertools.product((0, 1, M), (0, 2), (False, True)):
            for extra in (0, EN, EG, ES | SG, EN | ES | SG, EG | ES | SG):
                base = _answers(_solve(model, 24, members, samples, kernel, method, flags=extra, train=train))
                with_ = _answers(_solve(model, 24, members, samples, kernel, method, flags=extra | ENG, train=train))
                assert with_ == base, (method, kernel, members, samples, train, extra)
            if members <= 1:
                assert _answers(_solve(model, 24, members, samples, kernel, method, flags=ALL, train=train)) == \
                    _answers(_solve(model, 24, members, samples, kernel, method, flags=0, train=train))


def test_still_refused_under_all_three_flags():
    lib = _lib.lib()
    assert _answers(_solve(_model(), 24))[3] == 1
    # plans of the diffusion-net 4-row tiles: H = 128 nets, Milstein at H = 64, H = 16 / 32
    for model, method in ((_model(H=128), 0), (_model(H=128), 2), (_model(), 1), (_model(H=16), 2), (_model(H=32), 2),
                          (engine.model_struct(3, 64, 64, 2, 4, 19), 2)):
        assert engine.forward_kernel(_solve(model, 24, method=method, flags=EN, train=False)) == 'm4n', method
        _refused(_solve(model, 24, method=method), ('m4n', method))
    for method in (0, 2):
        # sample paths, with or without the sample flags
        for extra in (0, ES, ES | SG):
            _refused(_solve(_model(), 24, samples=2, method=method, flags=ALL | extra), ('samples', extra))
        # bf16 operands, the other kernel selectors
        _refused(_solve(_model(), 24, method=method, flags=ALL | _lib.FLAG_BF16_OPERANDS), 'bf16')
        _refused(_solve(_model(), 24, method=method, flags=ALL | _lib.FLAG_BF16_OPERANDS | _lib.FLAG_BF16_GRAD), 'bf16_grad')
        for kernel in ('generic', 'mfma16', 'mfma4'):
            _refused(_solve(_model(), 96 if kernel == 'mfma16' else 24, method=method, kernel=kernel), kernel)
        # a fused initial network, a supplied diffusion table, the accumulator column
        _refused(_solve(_model(), 24, method=method, z0_weight=P, z0_bias=P), 'z0_weight')
        _refused(_solve(_model(), 24, method=method, noise_table=P), 'noise_table')
        _refused(_solve(_model(), 24, method=method, kl_column1=3), 'kl_column1')
        # whole members of whole tiles
        for batch in (18, 25):
            _refused(_solve(_model(), batch, method=method), batch)
        # members = 0: no ensemble route - the flags are meaningful with members > 1 only and change no answer of one model, so the
        # descriptor answers as the ordinary differentiable solve it is (not 'none' / 0: that would break one-model training)
        one = _answers(_solve(_model(), 24, members=0, method=method))
        assert one == _answers(_solve(_model(), 24, members=0, method=method, flags=0)) and one[:4] == ('w4', 'w4', 'w4_fused', 1)
        # the field variants
        variant = _model()
        variant.activation, variant.drift_output, variant.diffusion_output, variant.time_feature = 1, 1, 2, 1
        _refused(_solve(variant, 24, method=method), 'variant')
        # dL/dcoeffs of an ensemble stays unsupported (the pair adjoints leave no delta planes)
        assert int(lib.snsde_coeff_gradients_workspace_bytes(C.byref(_backward(_solve(_model(), 24, method=method))))) == 0


def test_engine_queries_agree_with_the_library():
    grid = type('G', (), {'N': STEPS, 'T': 2})
    for method, code in (('euler', 0), ('srk', 2)):
        for model in (_model(), _model(5, 15, 1), _model(H=128), engine.model_struct(3, 64, 64, 2, 4, 17)):
            for flags in itertools.product((False, True), repeat=3):
                eg, en, eng = flags
                kw = dict(members=M, ensemble_grad=eg, ensemble_nets=en, ensemble_nets_grad=eng)
                bits = (EG if eg else 0) | (EN if en else 0) | (ENG if eng else 0)
                want = int(_lib.lib().snsde_backward_supported(C.byref(_solve(model, 24, method=code, flags=bits, train=False))))
                assert engine.backward_mode(model, 24, KNOTS, grid, method, global_rows=24, **kw) == want, (method, flags)
                desc = engine.query_descriptor(model, 24, KNOTS, STEPS, method, training=True, global_rows=24, **kw)
                assert int(desc.flags) & ALL == bits
                assert engine.forward_path(model, 24, KNOTS, STEPS, method, training=True, global_rows=24, **kw) == \
                    _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(desc))]
    q = dict(members=M, global_rows=24, training=True, ensemble_grad=True, ensemble_nets=True)
    assert engine.forward_path(_model(), 24, KNOTS, STEPS, ensemble_nets_grad=True, **q) == 'w4'
    assert engine.forward_path(_model(), 24, KNOTS, STEPS, **q) == 'none'
    assert engine.backward_mode(_model(), 24, KNOTS, grid, 'euler', members=M, ensemble_grad=True, ensemble_nets=True,
                                ensemble_nets_grad=True) == 1
    assert engine.backward_mode(_model(), 24, KNOTS, grid, 'euler', members=M, ensemble_grad=True, ensemble_nets=True) == 0
    assert engine.backward_mode(_model(), 24, KNOTS, grid, 'euler', members=0, ensemble_grad=True, ensemble_nets=True,
                                ensemble_nets_grad=True) == 1      # (one model: the flags are dropped)
    off = engine.query_descriptor(_model(), 24, KNOTS, STEPS, members=M, training=True, ensemble_grad=True, global_rows=24)
    assert engine.forward_kernel(off) == 'none'
    assert engine.forward_kernel(off, ensemble_nets=True, ensemble_nets_grad=True) == 'w4' and int(off.flags) & (EN | ENG) == 0


# ---- front end on CPU tensors ---------------------------------------------------------------------------------------------------

def test_option_checks():
    sdes, y0, times = _members(io=1, no=18)
    ts = torch.tensor([0., 2.2, 5.])
    for bad in (1, 'yes', None, 0):
        with pytest.raises(ValueError, match='ensemble_nets_grad must be a bool'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets_grad': bad})
        with pytest.raises(ValueError, match='ensemble_nets_grad must be a bool'):
            engine.check_ensemble_nets_grad(bad)
    assert engine.check_ensemble_nets_grad(True) is True and engine.check_ensemble_nets_grad(False) is False
    # alone, or with one of the two: ValueError naming what is missing
    with pytest.raises(ValueError, match=r"ensemble_nets'.*ensemble_grad'"):
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets_grad': True})
    with pytest.raises(ValueError, match="'ensemble_grad'") as exc:
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets_grad': True, 'ensemble_nets': True})
    assert "'ensemble_nets'" not in str(exc.value)
    with pytest.raises(ValueError, match="'ensemble_nets'") as exc:
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets_grad': True, 'ensemble_grad': True})
    assert "'ensemble_grad'" not in str(exc.value)
    S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5, options={'ensemble_nets_grad': False})      # (off: nothing to combine)
    with pytest.raises(NotImplementedError, match='strict'):      # CPU tensors have no fused solve
        S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=0.5,
                          options={'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True, 'strict': True})


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_cpu_ensemble_with_the_three_options_trains_like_the_members(method):
    sdes, y0, times = _members(io=1, no=18)      # M = 3, B = 4, H = 16
    B = 4
    ts = torch.tensor([0., 1.3, 2.2, 5.])
    for sde in sdes:
        sde.requires_grad_(True)
    opts = {'seed': 11, 'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True}
    ya = y0.clone().requires_grad_(True)
    got = S.sdeint_ensemble(sdes, ya, ts, method=method, dt=0.5, options=opts)
    cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(3))
    (got * cot).sum().backward()
    mine = [{n: p.grad.clone() for n, p in sde.named_parameters() if p.grad is not None} for sde in sdes]
    for sde in sdes:
        sde.zero_grad(set_to_none=True)
    yb = y0.clone().requires_grad_(True)
    ref = torch.stack([S.sdeint(sde, yb[m], ts, method=method, dt=0.5,
                                options={'seed': 11, 'row_offset': m * B, 'global_rows': M * B}) for m, sde in enumerate(sdes)], dim=1)
    (ref * cot).sum().backward()
    assert torch.equal(got, ref) and torch.equal(ya.grad, yb.grad)
    for gm, sde in zip(mine, sdes):
        assert gm and all(torch.equal(gm[n], p.grad) for n, p in sde.named_parameters() if p.grad is not None)
        assert float(gm['linear_out.weight'].abs().max()) > 0
    assert (mine[0]['linear_out.weight'] - mine[1]['linear_out.weight']).abs().max() > 1e-6


def test_cpu_ensemble_module_passes_the_option_through():
    from tests.test_ensemble_cpu import _wrappers
    models, coeffs, times = _wrappers(S.NeuralSDE)
    ens = S.Ensemble(models).eval()
    fi = torch.tensor([5, 3, 5, 2])
    with torch.no_grad():
        with pytest.raises(ValueError, match='ensemble_nets_grad must be a bool'):
            ens(times, (coeffs,), fi, options={'seed': 7, 'ensemble_nets_grad': 1})
        with pytest.raises(ValueError, match="'ensemble_grad'"):
            ens(times, (coeffs,), fi, options={'seed': 7, 'ensemble_nets': True, 'ensemble_nets_grad': True})
        got = ens(times, (coeffs,), fi, options={'seed': 7, 'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True})
        assert torch.equal(got, ens(times, (coeffs,), fi, options={'seed': 7}))
