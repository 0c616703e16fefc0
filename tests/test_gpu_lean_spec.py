"""The lean kernel's compile-time specialised instantiation (csrc/snsde_m4_kernel.h: CfgSpec) against its general instantiation
(SNSDE_FLAG_LEAN_GENERAL): states, saved activations, increments and the adjoint's gradients bit for bit, at the K2 (4, 17) and
GSDE (6, 17) shapes, batch sizes that are not a multiple of the 4-row tile, more steps than one Philox block and one step-table
chunk; and the route each takes."""
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from tests.helpers import make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('lean specialisation GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(300)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _flat(params, io, no, C, H):
    from tests.helpers import param_spec
    return torch.from_numpy(np.concatenate([params[n].reshape(-1) for n, _ in param_spec(io, no, 2, C, H)])).to(DEV)


def _calls(io, no, B, seed, train, L=150, ts=(0.0, 70.5, 149.0)):
    pr = make_problem(seed, io, no, 2, B, 128, 21, L)
    model = S.engine.model_struct(21, 128, 128, 2, io, no)
    grid = S.engine.step_grid(np.array(ts, np.float32), 1.0, pr['times'], torch.device(DEV))
    flat = _flat(pr['params'], io, no, 21, 128)
    coeffs, y0 = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['y0']).to(DEV)
    return [S.engine.SolveCall(model, flat, coeffs, grid, y0, method='euler', seed=seed, row_offset=3 * seed, save_traj=train,
                               save_dW=train, save_act=train, lean_general=general) for general in (False, True)]


@pytest.mark.parametrize('seed', [5, 1234])
@pytest.mark.parametrize('B', [37, 130, 1023])
@pytest.mark.parametrize('io', [4, 6])
def test_specialised_forward_is_bit_identical_to_the_general_one(io, B, seed):
    spec, gen = _calls(io, 17, B, seed, train=False)
    assert S.engine.lean_variant(spec) == 'specialised' and S.engine.lean_variant(gen) == 'general'
    a, b = spec.launch().clone(), gen.launch().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize('io,B,seed', [(4, 37, 7), (6, 130, 11), (4, 1021, 2024)])
def test_specialised_training_forward_and_adjoint_are_bit_identical(io, B, seed):
    outs = []
    for call in _calls(io, 17, B, seed, train=True):
        ys = call.launch().clone()
        g = torch.ones_like(ys) / ys.numel()
        g[-1] += torch.linspace(-1.0, 1.0, ys.shape[-1], device=DEV)
        adj, grad = S.engine.backward_with_gradients(call, g)[:2]
        outs.append((ys, call.traj.clone(), call.act_save.clone(), call.dW_out.clone(), adj.clone(), grad.clone()))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][5]).all()
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_excluded_cases_take_the_general_instantiation_and_match_it():
    # noise_option 7 (a y-dependent diffusion) and Milstein without a y factor in the table (noise_option 16) stay general
    for io, no, method in ((4, 7, 'euler'), (4, 16, 'milstein')):
        pr = make_problem(31, io, no, 2, 9, 128, 21, 12)
        model = S.engine.model_struct(21, 128, 128, 2, io, no)
        grid = S.engine.step_grid(np.array([0.0, 11.0], np.float32), 1.0, pr['times'], torch.device(DEV))
        call = S.engine.SolveCall(model, _flat(pr['params'], io, no, 21, 128), torch.from_numpy(pr['coeffs']).to(DEV), grid,
                                  torch.from_numpy(pr['y0']).to(DEV), method=method, seed=3)
        assert S.engine.forward_path(model, 9, 12, grid.N, method=method) == 'lean'
        assert S.engine.lean_variant(call) == 'general'
        assert torch.isfinite(call.launch()).all()
