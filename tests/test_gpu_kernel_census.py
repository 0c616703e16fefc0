"""Every compiled instantiation of the two-tile kernels on the GPU (run with -m gpu), at the smallest shapes: B = 3 (one ragged tile)
and B = 9 (two tile pairs, the second ragged), eight steps, one interpolated output.  tests/kernel_cases.py holds the cases and the
kernels they are meant to run; every launch here asserts its kernel on the descriptor it launched before anything is compared.

Forward (SNSDE_M4S2_LIST at H = 256, SNSDE_M4T_LIST at H = 128; inference and, where compiled, training mode): bit-equal to the
sibling kernel (SNSDE_FLAG_STREAM_ALL / no SNSDE_FLAG_TWO_TILE) under Philox and supplied increments, and held to the fp64 oracle
with the float32 oracle as yardstick (assert_parity).  Adjoint (SNSDE_M4S2_REV_LIST): every (NHID, GEO) pair against
fp64 autograd through the tensor loop (_check_backward, its constants) and bit-equal to the streamed adjoint, with and without
per-row outputs."""
import functools

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from tests import kernel_cases as K
from tests.helpers import assert_kernels, assert_parity, draw_dW, make_problem
from tests.test_gpu_parity import _check_backward, flat_params, h256_adjoint_arms, oracle_solve

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TS, DT = np.asarray(K.TS8, np.float32), K.DT8


@functools.lru_cache(maxsize=None)
def _problem(seed, io, no, NL, B, H, C, method):
    """One problem per (model, batch) with its supplied increments and both oracle solves on them: shared by the inference and the
    training case, never modified."""
    pr = make_problem(seed, io, no, NL, B, H, C, 9)
    dW = draw_dW(seed, TS, DT, B, H)
    return pr, dW, oracle_solve(pr, TS, DT, dW, method, np.float64)[0], oracle_solve(pr, TS, DT, dW, method, np.float32)[0]


def _forward_arms(seed, io, no, NL, B, H, C, method, train, flag, kernels):
    """Both arms of one two-tile forward case: `flag` -> (SolveCall keyword, its value in the sibling arm, in the two-tile arm),
    kernels = (sibling, two-tile).  Bit equality of every output and saved plane; the two-tile arm against the oracle."""
    pr, dW, ref64, cpu32 = _problem(seed, io, no, NL, B, H, C, method)
    model = S.engine.model_struct(C, H, H, NL, io, no)
    flat = flat_params(pr['params'], io, no, NL, C, H)
    grid = S.engine.step_grid(TS, DT, pr['times'], torch.device(DEV))
    name, sibling, two_tile = flag
    for supplied in (None, torch.from_numpy(dW).to(DEV)):
        outs = []
        for value, kernel in ((sibling, kernels[0]), (two_tile, kernels[1])):
            call = S.engine.SolveCall(model, flat, torch.from_numpy(pr['coeffs']).to(DEV), grid, torch.from_numpy(pr['y0']).to(DEV),
                                      dW=supplied, method=method, seed=11, kernel='mfma4', save_traj=train, save_dW=train, save_act=train,
                                      **{name: value})
            ys = call.launch().clone()
            assert_kernels(call, fwd=kernel)
            outs.append((ys, call.traj, call.act_save, call.dW_out))
        for x, y in zip(*outs):
            assert (x is None and y is None) or torch.equal(x, y)
        ys, _, _, dW_out = outs[1]
        if supplied is not None:
            assert_parity(ys.cpu().numpy(), ref64, cpu32, what=f'two-tile {kernels[1]} supplied increments')
        elif train:      # the Philox increments the kernel drew and saved: the oracle replays them
            drawn = dW_out.cpu().numpy()
            assert_parity(ys.cpu().numpy(), oracle_solve(pr, TS, DT, drawn, method, np.float64)[0],
                          oracle_solve(pr, TS, DT, drawn, method, np.float32)[0], what=f'two-tile {kernels[1]} Philox increments')
        else:
            assert torch.isfinite(ys).all()


@pytest.mark.parametrize('B', K.CENSUS_B)
@pytest.mark.parametrize('nhid,kuxt,train', K.M4S2_CASES)
def test_h256_two_tile_forward_of_every_instantiation(nhid, kuxt, train, B):
    io, no, NL, C, method = K.M4S2_MODELS[(nhid, kuxt)]
    _forward_arms(6600 + 10 * nhid + kuxt, io, no, NL, B, 256, C, method, train, ('stream_all', True, False),
                  ('lean_streamed_h256', 'lean_two_tile_h256'))


@pytest.mark.parametrize('B', K.CENSUS_B)
@pytest.mark.parametrize('nhid,kuxt,train', K.M4T_CASES)
def test_h128_two_tile_forward_of_every_instantiation(nhid, kuxt, train, B):
    io, no, NL, C, method = K.M4T_MODELS[(nhid, kuxt)]
    _forward_arms(6700 + 10 * nhid + kuxt, io, no, NL, B, 128, C, method, train, ('two_tile', False, True), ('lean', 'lean_two_tile_h128'))


@pytest.mark.parametrize('B', K.CENSUS_B)
@pytest.mark.parametrize('nhid,geo', K.M4S2_REV_LIST)
def test_h256_two_tile_adjoint_of_every_instantiation_matches_fp64_autograd(nhid, geo, B):
    io, no, NL, C, method, fwd = K.M4S2_REV_MODELS[(nhid, geo)]
    _check_backward(6800 + 10 * nhid + geo, io, no, NL, B, 256, C, 9, K.TS8, K.DT8, method, 'mfma4', strict=True,
                    expect=(fwd, 'two_tile_h256'))


@pytest.mark.parametrize('row_out', [False, True])
@pytest.mark.parametrize('B', K.CENSUS_B)
@pytest.mark.parametrize('nhid,geo', K.M4S2_REV_LIST)
def test_h256_two_tile_adjoint_of_every_instantiation_equals_the_streamed_one(nhid, geo, B, row_out):
    io, no, NL, C, method, fwd = K.M4S2_REV_MODELS[(nhid, geo)]
    h256_adjoint_arms(6900 + 10 * nhid + geo, io, no, NL, C, B, method, row_out, fwd)
