"""The decisions every route of sdeint shares, each read by one function of torchsde.py: the shard's first Philox row, the Philox
key, the increments of a solve (the only code that queries a Brownian object) and SnsdeError's "no kernel" answer.  No GPU."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from stable_neural_sdes_amd import torchsde as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, STEPS = 3, 5, 8


def test_row_offset_missing_and_none_are_not_given_and_an_explicit_value_wins():
    assert T._row_offset({}, 8) == 0 and T._row_offset({'row_offset': None}, 8) == 0
    for given in (0, 5, np.int64(24), torch.tensor(16)):
        got = T._row_offset({'row_offset': given}, 8)
        assert got == int(given) and type(got) is int


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, out_q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from stable_neural_sdes_amd import torchsde as TT
        out_q.put((rank, TT._row_offset({}, 6), TT._row_offset({'row_offset': None}, 6), TT._row_offset({'row_offset': 2}, 6)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_row_offset_defaults_to_rank_times_rows_under_gloo():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == [(0, 0, 0, 2), (1, 6, 6, 2)]


def test_a_sampled_call_refuses_a_row_offset_that_splits_a_group_of_paths():
    B, H = 4, 16
    m = S.Diffusion_model(3, H, H, 2, input_option=4, noise_option=17)
    times = torch.arange(5, dtype=torch.float32)
    m.set_X(torch.zeros(B, 4, 12), times)
    with torch.no_grad(), pytest.raises(ValueError, match='row_offset=3 must be a multiple of samples'):
        S.sdeint(m, torch.zeros(B, H), times, dt=1.0, method='euler', options={'samples': 2, 'row_offset': 3})
    with torch.no_grad():      # None is "not given": offset 0, a multiple of everything
        ys = S.sdeint(m, torch.zeros(B, H), times, dt=1.0, method='euler', options={'samples': 2, 'row_offset': None, 'seed': 1})
    assert ys.shape == (5, 2 * B, H)


def test_philox_key_passes_an_int_through_and_a_fresh_one_repeats_after_manual_seed():
    key = T._philox_key({'seed': np.int64(7)}, 'cpu')
    assert key == 7 and type(key) is int
    t = torch.tensor([9])
    assert T._philox_key({'seed': t}, 'cpu') is t      # (a device-resident key: as it is)
    torch.manual_seed(5)
    a, a2 = T._philox_key({}, 'cpu'), T._philox_key({'seed': None}, 'cpu')
    torch.manual_seed(5)
    b = T._philox_key({'seed': None}, 'cpu')
    assert type(a) is int and a == b and a2 != a


class _Field(torch.nn.Module):
    noise_type, sde_type = 'diagonal', 'ito'

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.b = torch.nn.Linear(COLS, COLS), torch.nn.Linear(COLS, COLS)

    def f(self, t, y):
        return torch.tanh(self.a(y)) * torch.cos(t)

    def g(self, t, y):
        return 0.3 * torch.sigmoid(self.b(y)) + 0.1 * torch.sin(t)


class _Recorder:
    """A Brownian object that records how it was asked."""

    def __init__(self, shape):
        self.shape, self.calls = shape, []

    def __call__(self, ta, tb=None, return_U=False, **kw):
        self.calls.append((ta, tb, return_U))
        n = float(len(self.calls))
        W = torch.full(self.shape, n)
        return (W, -W) if return_U else W


def _grid():
    return engine.StepGrid(np.array([0.0, 1.0], np.float32), 1.0 / STEPS, np.array([0.0, 1.0], np.float32), None)


@pytest.mark.parametrize('host_times', [False, True])
@pytest.mark.parametrize('method', T.METHODS)
def test_draw_increments_queries_bm_once_per_step_in_order_at_the_grids_times(method, host_times):
    grid, y0 = _grid(), torch.zeros(ROWS, COLS, dtype=torch.float64)
    assert grid.N == STEPS
    bm = _Recorder((ROWS, COLS))
    dW, dU = T._draw_increments(bm, grid, y0, method, host_times=host_times, philox=True)
    assert len(bm.calls) == STEPS
    for n, (ta, tb, return_U) in enumerate(bm.calls):
        assert return_U is (method == 'srk')
        assert torch.is_tensor(ta) and ta.device == y0.device and float(ta) == float(grid.t0[n]) and float(tb) == float(grid.t1[n])
    assert dW.shape == (STEPS, ROWS, COLS) and dW.dtype == y0.dtype
    assert [float(dW[n, 0, 0]) for n in range(STEPS)] == [float(n + 1) for n in range(STEPS)]      # (step order)
    assert (dU is None) == (method != 'srk') and (dU is None or torch.equal(dU, -dW))
    assert T._draw_increments(bm, grid, y0, method, dtype=torch.float32)[0].dtype == torch.float32


def test_draw_increments_without_bm_draws_philox_nothing_and_scalar_noise_one_column():
    grid, y0 = _grid(), torch.zeros(ROWS, COLS)
    assert T._draw_increments(None, grid, y0, 'srk', philox=True) == (None, None)
    dW, dU = T._draw_increments(None, grid, y0, 'euler', seed=4, scalar=True)
    assert dW.shape == (STEPS, ROWS, 1) and dU is None
    dW, dU = T._draw_increments(None, grid, y0, 'srk', seed=4)
    assert dW.shape == dU.shape == (STEPS, ROWS, COLS)
    assert torch.equal(dW, T._draw_increments(None, grid, y0, 'srk', seed=4)[0])


@pytest.mark.parametrize('method', T.METHODS)
def test_the_loop_on_a_seeded_draw_is_the_loop_fed_the_same_draw(method):
    sde, ts = _Field(), torch.tensor([0.0, 1.0])
    y0 = torch.linspace(-1, 1, ROWS * COLS).reshape(ROWS, COLS)
    with torch.no_grad():
        whole = S.sdeint(sde, y0, ts, method=method, dt=1.0 / STEPS, options={'backend': 'torch', 'seed': 11})
        drawn = T._DrawnIncrements(*T._draw_increments(None, _grid(), y0, method, seed=11))
        fed = T._sdeint_torch(sde, y0, ts, drawn, method, 1.0 / STEPS, {}, None)
    assert drawn.n == STEPS
    assert whole.shape == (2, ROWS, COLS) and torch.equal(whole, fed)
    assert float((whole[-1] - y0).abs().max()) > 1e-3      # (a solve that moved)


def test_no_kernel_is_true_for_exactly_the_two_codes_of_the_header():
    text = open(os.path.join(ROOT, 'include', 'snsde.h')).read()
    codes = {name: int(val) for name, val in re.findall(r'\b(SNSDE_ERR_\w+)\s*=\s*(-\d+)', text)}
    assert len(codes) >= 10 and codes['SNSDE_ERR_UNSUPPORTED'] == _lib.SNSDE_ERR_UNSUPPORTED and codes['SNSDE_ERR_LDS'] == _lib.SNSDE_ERR_LDS
    for name, code in codes.items():
        assert _lib.SnsdeError(code).no_kernel is (name in ('SNSDE_ERR_UNSUPPORTED', 'SNSDE_ERR_LDS')), name
