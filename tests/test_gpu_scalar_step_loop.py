"""The lean forward kernels' step loop runs on a scalar bound and counter (csrc/snsde_m4_kernel.h, snsde_m4s_kernel.h,
snsde_m4s2_kernel.h, snsde_m4t_kernel.h: n_end = readfirstlane(out_step[ko])).  What that touches is how the steps are cut into
output segments, so this file pins the property that must not depend on it: with every output time on the step grid, the states
are bit-identical whatever the output schedule (the step body never reads the output index, and an on-grid output is a copy of
the state).  133 steps: past the 128-row refill of the step table, not a multiple of the four-step spline batch nor of the
16-step Philox block; 6 rows: one full 4-row tile and a partial one.  Plus the two ends of the loop bounds (a solve of one step, a
first output right after step 0) against the fp64 oracle."""
import signal

import numpy as np
import pytest
import torch

from oracle import sde_oracle as O
from stable_neural_sdes_amd import engine
from tests.helpers import assert_parity, draw_dW, make_problem, param_spec

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

N, B = 133, 6
SCHEDULES = {'ends': [0, N], 'every': list(range(N + 1)), 'seventh': list(range(0, N, 7)) + [N]}

# route -> H, C, SolveCall arguments, the forward kernel and the lean variant the launch must report
ROUTES = {
    'specialised': (128, 21, dict(), 'lean', 'specialised'),
    'general': (128, 21, dict(lean_general=True), 'lean', 'general'),
    'two_tile': (128, 21, dict(kernel='mfma4', two_tile=True), 'lean_two_tile_h128', 'none'),
    'bf16': (128, 21, dict(precision='bf16'), 'lean_bf16', None),
    'h256': (256, 14, dict(kernel='mfma4'), 'lean_two_tile_h256', 'none'),
    'h256_stream_all': (256, 14, dict(kernel='mfma4', stream_all=True), 'lean_streamed_h256', 'none'),
}


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('scalar step loop GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


_PROBLEMS = {}


def _problem(H, C, L):
    """K2's architecture ((4, 17), two layers) on L knots, one per (H, C, L); its device tensors are shared and never written."""
    key = (H, C, L)
    if key not in _PROBLEMS:
        pr = make_problem(5, 4, 17, 2, B, H, C, L)
        flat = torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in param_spec(4, 17, 2, C, H)])).to(DEV)
        _PROBLEMS[key] = (pr, engine.model_struct(C, H, H, 2, 4, 17), flat, torch.from_numpy(pr['coeffs']).to(DEV),
                          torch.from_numpy(pr['y0']).to(DEV))
    return _PROBLEMS[key]


def _call(route, ts, L=N + 1, train=False, dW=None, **more):
    H, C, kw, fwd, variant = ROUTES[route]
    pr, model, flat, coeffs, y0 = _problem(H, C, L)
    grid = engine.step_grid(np.array(ts, np.float32), 1.0, pr['times'], torch.device(DEV))
    call = engine.SolveCall(model, flat, coeffs, grid, y0, dW=dW, method='euler', seed=20261019, row_offset=3,
                            save_traj=train, save_dW=train, save_act=train, **kw, **more)
    assert engine.forward_kernel(call) == fwd, (route, engine.forward_kernel(call, keys=True))
    if variant is not None:
        assert engine.lean_variant(call) == variant, (route, engine.lean_variant(call))
    return call, grid, pr


@pytest.mark.parametrize('route', list(ROUTES))
def test_states_do_not_depend_on_the_output_schedule(route):
    ys = {}
    for name, ts in SCHEDULES.items():
        call, grid, _ = _call(route, ts)
        assert grid.N == N and grid.T == len(ts)
        assert grid.out_step.tolist() == [t - 1 for t in ts[1:]] and (grid.out_w[:, 0] == 0).all()      # every output on the grid
        ys[name] = call.launch().clone()
    torch.cuda.synchronize()
    every = ys['every']
    assert torch.isfinite(every).all()
    assert not torch.equal(every[1], every[N])      # (the solve moves: equal planes below are not a stuck state)
    assert torch.equal(ys['ends'][0], every[0]) and torch.equal(ys['ends'][1], every[N])
    idx = torch.tensor(SCHEDULES['seventh'], device=DEV)
    assert torch.equal(ys['seventh'], every[idx])
    assert torch.equal(ys['seventh'][-1], ys['ends'][1])


def test_training_planes_do_not_depend_on_the_output_schedule():
    planes = {}
    for name in ('ends', 'every'):
        call, grid, _ = _call('specialised', SCHEDULES[name], train=True)
        assert grid.N == N
        ys = call.launch().clone()
        planes[name] = (ys, call.traj.clone(), call.act_save.clone(), call.dW_out.clone())
    torch.cuda.synchronize()
    (ya, *a), (yb, *b) = planes['ends'], planes['every']
    assert torch.equal(ya[1], yb[N]) and torch.equal(a[0][N], yb[N])      # (the trajectory's last plane is the last state)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)


# the two ends of the loop bounds: one step in all (out_step = [0]), and a first output right after step 0 (out_step[0] = 0)
@pytest.mark.parametrize('ts', [(0.0, 1.0), (0.0, 1.0, 5.0)], ids=['one_step', 'first_output_after_step_0'])
@pytest.mark.parametrize('route', ['specialised', 'general_supplied', 'two_tile', 'h256', 'h256_stream_all'])
def test_shortest_segments_against_the_oracle(route, ts):
    L = 8
    ts = np.array(ts, np.float32)
    if route == 'general_supplied':      # supplied increments: the general instantiation, inference mode
        H, C = ROUTES['general'][:2]
        pr = _problem(H, C, L)[0]
        dW = draw_dW(9, ts, 1.0, B, H)
        call, grid, _ = _call('general', ts, L=L, dW=torch.from_numpy(dW).to(DEV))
        got = call.launch()
    else:                                # in-kernel Philox: training mode hands the increments out for the oracle
        H, C = ROUTES[route][:2]
        call, grid, pr = _call(route, ts, L=L, train=True)
        got = call.launch()
        dW = call.dW_out.cpu().numpy()
    torch.cuda.synchronize()
    assert grid.N == int(ts[-1]) and grid.out_step[0] == 0
    ref64, _ = O.solve_diffusion_model(pr['params'], 4, 17, pr['coeffs'], pr['times'], pr['y0'], ts, 1.0, dW, dtype=np.float64)
    assert_parity(got.cpu().numpy(), ref64, what=f'{route} ts={ts.tolist()}')
