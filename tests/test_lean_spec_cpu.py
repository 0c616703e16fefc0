"""Which instantiation of the lean kernel a forward takes (snsde_lean_variant, host-only): the compile-time specialised one
(csrc/snsde_m4_kernel.h: CfgSpec) at the K2 and GSDE shapes, the general one for every option the specialisation excludes and
under SNSDE_FLAG_LEAN_GENERAL.  The path reported by snsde_forward_path stays 'lean' either way.  No GPU compute."""
import ctypes as C

import pytest

from stable_neural_sdes_amd import _lib, engine


def _query(io=4, no=17, batch=1024, method='euler', dW=False, flags=0, train=False, hidden=128, nl=2, channels=21, **model_kw):
    m = engine.model_struct(channels, hidden, hidden, nl, io, no)
    for k, v in model_kw.items():
        setattr(m, k, v)
    s = _lib.Solve()
    s.model = m
    s.batch, s.knots, s.n_steps, s.n_out = batch, 101, 100, 2
    s.method = {'euler': _lib.EULER, 'milstein': _lib.MILSTEIN, 'srk': _lib.SRK}[method]
    s.kernel = _lib.KERNELS['auto']
    s.flags = flags
    s.dW = C.c_void_p(16) if dW else None
    if train:
        s.traj, s.act_save = C.c_void_p(16), C.c_void_p(32)
    lib = _lib.lib()
    return _lib.PATHS[lib.snsde_forward_path(C.byref(s))], _lib.LEAN_VARIANTS[lib.snsde_lean_variant(C.byref(s))]


@pytest.mark.parametrize('train', [False, True])
@pytest.mark.parametrize('io', [4, 6, 2])
def test_k2_and_gsde_shapes_take_the_specialised_instantiation(io, train):
    assert _query(io=io, train=train) == ('lean', 'specialised')
    assert _query(io=io, batch=37, train=train) == ('lean', 'specialised')


@pytest.mark.parametrize('no', [3, 6, 11, 13])
def test_other_table_times_y_noise_options_are_specialised(no):
    assert _query(no=no) == ('lean', 'specialised')


@pytest.mark.parametrize('case', [
    dict(no=7),                           # y-dependent diffusion
    dict(no=16),                          # table noise without the y factor
    dict(method='milstein'),
    dict(no=12, method='milstein'),       # Milstein without a y factor
    dict(dW=True),                        # supplied increments
    dict(io=5),                           # no control path in the first layer
    dict(nl=1),                           # a shape without a specialised instantiation
    dict(hidden=64),
    dict(flags=_lib.FLAG_LEAN_GENERAL),
])
def test_excluded_cases_keep_the_general_instantiation(case):
    assert _query(**case) == ('lean', 'general')


def test_field_variants_keep_the_general_instantiation():
    assert _query(activation=1) == ('lean', 'general')          # SNSDE_ACT_LIPSWISH
    assert _query(drift_output=2)[1] != 'specialised'           # SNSDE_DRIFT_TIMES_Y


def test_other_kernels_report_none():
    assert _query(method='srk')[1] == 'none'
    assert _query(flags=_lib.FLAG_BF16_OPERANDS) == ('lean-bf16', 'none')
