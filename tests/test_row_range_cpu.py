"""The range of the global row on the host (include/snsde.h: snsde_solve.row_offset): the first Philox counter word is the global row
in 32 bits, so a call whose rows leave [0, 2^32) is refused - SNSDE_ERR_DIMS from the library with or without global_rows,
ValueError from engine.check_row_offset, the sdeint options and the oracle - instead of silently re-drawing the paths of rows 0 ..
No GPU compute."""
import ctypes as C

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import elementwise_model, net_model
from tests.test_step_offset_cpu import ERR_DIMS, TS, Stub, _launch_rc, _model, _solve

BATCH = 8
LAST = 2 ** 32 - BATCH      # the last legal offset: its last row is 2^32 - 1

# descriptor family -> (model, kernel selector, method, forward kernel the plan names)
DESCRIPTORS = {'lean': (elementwise_model(32), 'auto', _lib.EULER, 'lean'),
               'generic': (elementwise_model(32), 'generic', _lib.EULER, 'generic'),
               'wave pair': (net_model(), 'w4', _lib.EULER, 'w4')}


def _desc(family, **kw):
    model, kernel, method, _ = DESCRIPTORS[family]
    return _solve(model, batch=BATCH, method=method, kernel=_lib.KERNELS[kernel], **kw)


@pytest.mark.parametrize('family', list(DESCRIPTORS))
def test_the_library_refuses_rows_outside_32_bits(family):
    assert engine.forward_kernel(_desc(family)) == DESCRIPTORS[family][3]
    accepted = _launch_rc(_desc(family))      # (a valid descriptor without a workspace: SNSDE_ERR_WORKSPACE, past every check of the row)
    assert accepted not in (0, ERR_DIMS)
    for ok in (0, 40, 2 ** 31 - 4, 2 ** 31, LAST):
        assert _launch_rc(_desc(family, row_offset=ok)) == accepted, ok
        assert _launch_rc(_desc(family, row_offset=ok), 5) == accepted, ok
    for bad in (LAST + 1, 2 ** 32, 2 ** 40, -1, -BATCH, -2 ** 40):
        assert _launch_rc(_desc(family, row_offset=bad)) == ERR_DIMS, bad
        assert _launch_rc(_desc(family, row_offset=bad), 5) == ERR_DIMS, bad
    # ... independently of global_rows: a whole problem of more than 2^32 rows does not make its last shards legal
    assert _launch_rc(_desc(family, row_offset=LAST, global_rows=2 ** 32)) == accepted
    assert _launch_rc(_desc(family, row_offset=LAST, global_rows=2 ** 33)) == accepted
    assert _launch_rc(_desc(family, row_offset=LAST + 1, global_rows=2 ** 33)) == ERR_DIMS
    assert _launch_rc(_desc(family, row_offset=2 ** 32, global_rows=2 ** 33)) == ERR_DIMS


def test_sample_paths_count_rows_in_paths():
    """samples = S: batch and row_offset count paths, so 2^32 / S input rows is the limit."""
    s = _desc('lean', samples=4, row_offset=LAST)
    assert _launch_rc(s) == _launch_rc(_desc('lean', samples=4))
    assert _launch_rc(_desc('lean', samples=4, row_offset=LAST + 4)) == ERR_DIMS


def test_the_abi_did_not_move():
    assert C.sizeof(_lib.Solve) == 304 and _lib.lib().snsde_version() == 2


def test_check_row_offset():
    assert engine.check_row_offset(0, 8) == 0 and engine.check_row_offset(np.int64(40), 8) == 40
    assert engine.check_row_offset(LAST, BATCH) == LAST and engine.check_row_offset(2 ** 32 - 1, 1) == 2 ** 32 - 1
    for bad, batch in ((LAST + 1, BATCH), (2 ** 32, 1), (-1, 8), (-2 ** 33, 8)):
        with pytest.raises(ValueError, match='row_offset.*2\\*\\*32'):
            engine.check_row_offset(bad, batch)


@pytest.mark.parametrize('bad', [-1, 2 ** 32 - 3, 2 ** 32, 2 ** 40])
def test_sdeint_refuses_the_option(bad):
    m, pr = _model()      # four rows
    y0 = torch.from_numpy(pr['y0'])
    with pytest.raises(ValueError, match='row_offset'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', bm=Stub(), options={'row_offset': bad})
    with pytest.raises(ValueError, match='row_offset'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', bm=Stub(), options={'row_offset': bad, 'global_rows': 2 ** 41})
    with pytest.raises(ValueError, match='row_offset'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', bm=Stub(), options={'row_offset': bad, 'backend': 'torch'})
    with pytest.raises(ValueError, match='row_offset'):
        S.sdeint_ensemble([m, m], y0[None].repeat(2, 1, 1), TS, dt=0.25, method='euler', bm=Stub(), options={'row_offset': bad})


def test_sdeint_accepts_the_last_legal_rows():
    m, pr = _model()
    y0 = torch.from_numpy(pr['y0'])
    whole = S.sdeint(m, y0, TS, dt=0.25, method='euler', bm=Stub())
    assert torch.equal(S.sdeint(m, y0, TS, dt=0.25, method='euler', bm=Stub(), options={'row_offset': 2 ** 32 - 4}), whole)
    # under samples the rows are paths: 4 rows x 2 paths end at 2^32
    with pytest.raises(ValueError, match='row_offset'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', bm=Stub((8, 16)), options={'row_offset': 2 ** 32 - 4, 'samples': 2})
