"""The exact kernel a plan runs (snsde_forward_kernel / snsde_backward_kernel, host-only) and the census of the kernel-specific tests.

Consistency: over a descriptor sweep the two queries agree with every older query that reports part of the same decision
(snsde_forward_path as snsde_mfma_path folds the kernels, snsde_lean_variant, snsde_backward_supported, the delta slots of
snsde_save_layout).  Census: every case of tests/kernel_cases.py - the cases of the GPU tests that are about one kernel - plans
the kernels it names, and together the cases cover every value of both queries and every compiled instantiation of the two-tile
kernels.  There is no allow-list: a kernel a plan can reach, or an instantiation that is compiled, has a case.  No GPU compute."""
import ctypes as C
import itertools

import pytest

from stable_neural_sdes_amd import _lib, engine
from tests import kernel_cases as K

# forward kernel -> family, as csrc/snsde_mfma.hip snsde_mfma_path states it (SRK: the general and the net kernels report 'mfma-srk')
FAMILY = {'none': 'none', 'generic': 'generic', 'generic_srk': 'generic-srk', 'w4': 'w4', 'm4n': 'mfma4', 'lean': 'lean',
          'lean_two_tile_h128': 'lean', 'lean_two_tile_h256': 'lean-streamed', 'lean_streamed_h256': 'lean-streamed',
          'general_m4': 'mfma4', 'general_m16': 'mfma16', 'lean_bf16': 'lean-bf16'}
FLAG_SETS = (0, _lib.FLAG_STREAM_ALL, _lib.FLAG_TWO_TILE, _lib.FLAG_LEAN_GENERAL, _lib.FLAG_BF16_OPERANDS,
             _lib.FLAG_BF16_OPERANDS | _lib.FLAG_BF16_GRAD)
HS, CS, BATCHES = (16, 32, 64, 128, 256), (0, 3, 14, 21, 40, 69), (9, 1024, 8192)


def _desc(io, no, NL, H, C_, method, train, kernel, flags, batch):
    s = _lib.Solve()
    s.model = engine.model_struct(C_, H, H, NL, io, no)
    s.batch, s.knots, s.n_steps, s.n_out = batch, 9, 8, 4
    s.method, s.kernel, s.flags = method, kernel, flags
    p = C.c_void_p(256)      # (no host-only query dereferences a pointer of the descriptor)
    if train:
        s.traj = s.act_save = s.dW_out = p
        if method == _lib.SRK:
            s.stage_save = s.dU_out = p
    if method == _lib.SRK:
        s.srk_tab = p
    return s


def _answers(s):
    lib = _lib.lib()
    fk, nhid, kuxt = engine.forward_kernel(s, keys=True)
    a, p, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = lib.snsde_save_layout(C.byref(s), C.byref(a), C.byref(p), C.byref(d))
    return (fk, nhid, kuxt, _lib.PATHS[lib.snsde_forward_path(C.byref(s))], _lib.LEAN_VARIANTS[lib.snsde_lean_variant(C.byref(s))],
            engine.backward_kernel(s), lib.snsde_backward_supported(C.byref(s)), rc, d.value)


def _sweep():
    """(io, no, NL, H, C, method, train, kernel selector, flags, batch): the full cross of options, sizes, methods, planes, selectors
    and flag sets with NL, C and the batch rotating through their values, then every NL x C at the two sizes that have two-tile
    kernels on the 4-row-tile selector."""
    i = 0
    for io, no, H, method, train, kernel, flags in itertools.product(range(7), range(20), HS, (0, 1, 2), (False, True), range(6), FLAG_SETS):
        i += 1
        yield io, no, 1 + i % 4, H, CS[(i // 4) % 6], method, train, kernel, flags, BATCHES[(i // 5) % 3]
    for io, no, NL, H, C_, train, flags in itertools.product(range(7), range(20), (1, 2, 3, 4), (128, 256), CS, (False, True), FLAG_SETS):
        yield io, no, NL, H, C_, (io + no + NL) % 2, train, _lib.KERNELS['mfma4'], flags, 9


@pytest.fixture(scope='module')
def sweep():
    """One pass over the sweep: every inconsistency, and what the plans reached."""
    bad, fwd, rev, m4s2, m4t, m4s2_rev, n = [], set(), set(), set(), set(), set(), 0
    for key in _sweep():
        io, no, NL, H, C_, method, train = key[:7]
        fk, nhid, kuxt, path, lean, bk, mode, rc, dslots = _answers(_desc(*key))
        n += 1
        srk_mfma = method == _lib.SRK and fk in ('m4n', 'general_m4', 'general_m16')
        ok = (path == ('mfma-srk' if srk_mfma else FAMILY[fk]) and (lean != 'none') == (fk == 'lean') and
              (bk == 'none') == (mode == 0) and (bk == 'generic') == (mode == 2) and
              ((nhid, kuxt) == (-1, -1)) == (fk in ('none', 'generic', 'generic_srk')) and (nhid in (-1, NL - 1)) and
              (bk != 'w4_fused' or rc == 0) and (rc != 0 or (dslots == 0) == (bk == 'w4_fused')))
        if not ok and len(bad) < 20:
            bad.append((key, fk, nhid, kuxt, path, lean, bk, mode, rc, dslots))
        fwd.add(fk)
        rev.add(bk)
        if fk == 'lean_two_tile_h256':
            m4s2.add((nhid, kuxt, int(train)))
        if fk == 'lean_two_tile_h128':
            m4t.add((nhid, kuxt, int(train)))
        if bk == 'two_tile_h256':
            m4s2_rev.add((NL - 1, int(io in (5, 6))))
    return dict(bad=bad, fwd=fwd, rev=rev, m4s2=m4s2, m4t=m4t, m4s2_rev=m4s2_rev, n=n)


def _compiled(lst):
    """(NHID, KUXT, training) triples an instantiation list stands for: inference always, training where SAVE is 1."""
    return {(nhid, kuxt, t) for nhid, kuxt, save in lst for t in ((0, 1) if save else (0,))}


def test_the_kernel_queries_agree_with_the_older_queries_over_the_sweep(sweep):
    assert sweep['n'] > 200000
    assert not sweep['bad'], sweep['bad']


def test_the_sweep_reaches_every_kernel_and_every_compiled_instantiation(sweep):
    """No value of either query and no entry of an instantiation list is dead - and no plan names a two-tile instantiation that is not
    compiled (the launch would have nothing to dispatch to)."""
    assert sweep['fwd'] == set(_lib.FWD_KERNELS)
    assert sweep['rev'] == set(_lib.REV_KERNELS)
    assert sweep['m4s2'] == _compiled(K.M4S2_LIST)
    assert sweep['m4t'] == _compiled(K.M4T_LIST)
    assert sweep['m4s2_rev'] == set(K.M4S2_REV_LIST)


CENSUS = K.census()


def test_every_case_plans_the_kernels_it_names():
    wrong = []
    for c in CENSUS:
        s = K.descriptor(c)
        got = (engine.forward_kernel(s), engine.backward_kernel(s))
        if got[0] != c.fwd or (c.rev is not None and got[1] != c.rev):
            wrong.append((c.test, c.kernel, dict(stream_all=c.stream_all, two_tile=c.two_tile, train=c.train, supplied=c.supplied),
                          'meant', (c.fwd, c.rev), 'plans', got))
    assert not wrong, wrong


def test_the_cases_cover_every_kernel():
    assert {c.fwd for c in CENSUS} == set(_lib.FWD_KERNELS)
    assert {c.rev for c in CENSUS if c.rev is not None} == set(_lib.REV_KERNELS)


def test_the_cases_cover_every_compiled_two_tile_instantiation():
    m4s2, m4t, rev = set(), set(), set()
    for c in CENSUS:
        s = K.descriptor(c)
        fk, nhid, kuxt = engine.forward_kernel(s, keys=True)
        if fk == c.fwd == 'lean_two_tile_h256':
            m4s2.add((nhid, kuxt, int(c.train)))
        if fk == c.fwd == 'lean_two_tile_h128':
            m4t.add((nhid, kuxt, int(c.train)))
        if c.rev == 'two_tile_h256' and engine.backward_kernel(s) == c.rev:
            rev.add((c.NL - 1, int(c.io in (5, 6))))
    assert m4s2 == _compiled(K.M4S2_LIST), sorted(_compiled(K.M4S2_LIST) - m4s2)
    assert m4t == _compiled(K.M4T_LIST), sorted(_compiled(K.M4T_LIST) - m4t)
    assert rev == set(K.M4S2_REV_LIST), sorted(set(K.M4S2_REV_LIST) - rev)


def test_sibling_arms_name_two_different_kernels():
    """The bit-identity tests compare two arms of one case; where the case is meant to be a real comparison the arms differ in the
    kernel, and the cases that decline to the sibling say so."""
    by_case = {}
    for c in CENSUS:
        if c.test.startswith(('h256 forward', 'h128 case', 'm4s2 (', 'm4t (')):
            by_case.setdefault((c.test, c.B, c.train, c.supplied), set()).add(c.fwd)
        if c.test.startswith(('h256 adjoint', 'h256 chunks')) or (c.test.startswith('m4s2 rev') and 'autograd' not in c.test):
            by_case.setdefault((c.test, c.B, c.row_out, c.supplied), set()).add(c.rev)
    declines = {f'h256 forward case {ci} train={train}' for ci, train in K.H256_FWD_DECLINES}
    assert by_case and declines
    for key, kernels in by_case.items():
        assert len(kernels) == (1 if key[0] in declines else 2), (key, kernels)


def test_the_lists_are_the_ones_compiled():
    """The lists written out in tests/kernel_cases.py against the source (the full build's branch of each #if)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
    for fname, macro, want in (('snsde_m4s2_h256.hip', 'SNSDE_M4S2_LIST', K.M4S2_LIST), ('snsde_m4t_h128.hip', 'SNSDE_M4T_LIST', K.M4T_LIST),
                               ('snsde_m4s2_rev_h256.hip', 'SNSDE_M4S2_REV_LIST', K.M4S2_REV_LIST)):
        defs = re.findall(r'#define %s\(X\) (.*)' % macro, open(os.path.join(csrc, fname)).read())
        got = tuple(tuple(int(v) for v in e.split(',')) for e in re.findall(r'X\(([^)]*)\)', defs[-1]))
        assert got == tuple(want), (fname, got)


def test_helpers_take_a_call_or_a_descriptor():
    s = K.descriptor(K.launch('K5', 4, 17, 2, 9, 256, 14, 9, K.TS8, K.DT8, 'milstein', 'mfma4', train=True))

    class Call:
        desc = s
    assert engine.forward_kernel(Call) == engine.forward_kernel(s) == 'lean_two_tile_h256'
    assert engine.forward_kernel(s, keys=True) == ('lean_two_tile_h256', 1, 1)
    assert engine.backward_kernel(Call) == engine.backward_kernel(s) == 'two_tile_h256'
    lib = _lib.lib()
    assert lib.snsde_forward_kernel(C.byref(s), None, None) == _lib.FWD_KERNELS.index('lean_two_tile_h256')      # (NULL out-pointers)
    assert lib.snsde_forward_kernel(None, None, None) == 0 and lib.snsde_backward_kernel(None) == 0


def test_the_poisoned_allocation_tables_name_every_forward_and_every_adjoint_kernel():
    """tests/test_gpu_poisoned_allocations.py runs STEP_OFFSET_CASES (inference) and POISONED_TRAINING_CASES (training): every row
    plans the kernels it names, the first table covers every forward kernel, the second every adjoint kernel, and only the
    wave-pair adjoint - which sums the weight gradients itself - leaves no delta planes for a coefficient gradient."""
    for c in K.STEP_OFFSET_CASES + K.POISONED_TRAINING_CASES:
        s = K.descriptor(c)
        assert engine.forward_kernel(s) == c.fwd, (c.test, engine.forward_kernel(s, keys=True))
        if c.train:
            assert engine.backward_kernel(s) == c.rev, (c.test, engine.backward_kernel(s))
            assert (K.delta_slots(c) == 0) == (c.rev == 'w4_fused'), (c.test, K.delta_slots(c))      # (w4_fused: no planes, no dL/d coeffs)
    assert not any(c.train or c.supplied for c in K.STEP_OFFSET_CASES) and all(c.train and not c.supplied for c in K.POISONED_TRAINING_CASES)
    assert {c.fwd for c in K.STEP_OFFSET_CASES} == set(_lib.FWD_KERNELS) - {'none'}
    assert {c.rev for c in K.POISONED_TRAINING_CASES} == set(_lib.REV_KERNELS) - {'none'}
    assert len({c.test for c in K.POISONED_TRAINING_CASES}) == len(K.POISONED_TRAINING_CASES)
