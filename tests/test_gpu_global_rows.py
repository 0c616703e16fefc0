"""options={'global_rows': N} on the GPU: the eight N / 8-row shards of a problem, solved one after the other with their
row_offset, reproduce the N-row solve bit for bit where the planner alone would have put them on other tiles (elementwise
diffusions at the batch where `auto` leaves the 4-row tiles; the H = 64 diffusion net, whose 1024-row shards would take the wave
pairs) - states, trajectory, dL/dy0 - and the parameter gradients within the margin of tests/test_gpu_backward_sizes.py.  Every
bitwise case also asserts that the same shards WITHOUT the option differ, so that no case compares a kernel with itself."""
import functools
import signal

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.global_rows_cases import CHANNELS, FOUR_ROW, KNOTS, SHARDS, elementwise_model, flip_batch, net_model, path
from tests.helpers import make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
SEED = 20261018
# parameter gradients: shard sums are added in another order than the in-kernel partial sums.  The measure and the margin are those
# of the backward parity tests (tests/bigcase.py: max |err| / max |ref| and mean |err| / mean |ref|; 4e-5 where the rows that a
# relu kink moves are set aside - here the states are equal bit for bit, so no row moves and none is set aside)
GRAD_TOL = 4e-5


@pytest.fixture(autouse=True)
def _time_limit():
    """every test of this file under its own time limit"""
    def fire(*_):
        raise TimeoutError('global_rows GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(300)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


# name -> (io, no, H, rows, solver steps)
def _case(name):
    if name == 'net':
        return 1, 18, 64, 8192, 3
    H = int(name[1:])
    return 4, 17, H, flip_batch(H), KNOTS - 1


@functools.lru_cache(maxsize=None)
def _problem(name):
    io, no, H, N, steps = _case(name)
    pr = make_problem(SEED & 0xFFFF, io, no, 2, N, H, CHANNELS, KNOTS, nan_frac=0.0)
    m = S.Diffusion_model(CHANNELS, H, H, 2, input_option=io, noise_option=no)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(DEV)
    t = {k: torch.from_numpy(pr[k]).to(DEV) for k in ('coeffs', 'times', 'y0')}
    ts = t['times'][[0, 2, steps]] if steps > 2 else t['times'][[0, steps]]
    return m, t, ts, N


def _solve(name, method, lo, hi, grad=False, **options):
    """Rows lo .. hi - 1 of the problem as one solve; Philox increments of the global rows.  -> (ys, traj or y0 leaf)"""
    m, t, ts, N = _problem(name)
    m.set_X(t['coeffs'][lo:hi].contiguous(), t['times'])
    y0 = t['y0'][lo:hi].clone().requires_grad_(grad)
    opts = dict(seed=SEED, row_offset=lo, strict=True, **options)
    if grad:
        return S.sdeint(m, y0, ts, dt=1.0, method=method, options=opts), y0
    with torch.no_grad():
        ys = S.sdeint(m, y0, ts, dt=1.0, method=method, options=dict(opts, save_traj=True))
    return ys, m.last_trajectory


@functools.lru_cache(maxsize=None)
def _whole(name, method):
    _, _, _, N = _problem(name)
    ys, traj = _solve(name, method, 0, N)
    return ys.clone(), traj.clone()


def _shards(name, method, **options):
    N = _problem(name)[3]
    n = N // SHARDS
    assert n * SHARDS == N
    parts = [_solve(name, method, r * n, (r + 1) * n, **options) for r in range(SHARDS)]
    return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)


def _check_forward(name, method):
    N = _problem(name)[3]
    ys, traj = _whole(name, method)
    ys_g, traj_g = _shards(name, method, global_rows=N)
    ys_l, traj_l = _shards(name, method)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ys).all()) and float(ys[-1].abs().max()) > 0
    assert torch.equal(ys_g, ys) and torch.equal(traj_g, traj)
    assert not torch.equal(ys_l, ys) and not torch.equal(traj_l, traj)      # the same shards on their own plan: other tiles


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_elementwise_shards_reproduce_the_whole_solve_bitwise(method):
    """H = 128 at the batch where `auto` leaves the 4-row tiles (the SRK variant has its 16-row flavour at H = 64 / 128 and
    changes at the same batch there; its path name does not tell the tiles, the 'differs without' assertion does)."""
    model, N = elementwise_model(128), flip_batch(128)
    assert path(model, N) == 'mfma16' and path(model, N // SHARDS) in FOUR_ROW
    _check_forward('H128', method)


def test_h256_shards_reproduce_the_whole_solve_bitwise():
    """H = 256 changes tiles at another ratio (streamed weights), so at a batch of its own."""
    assert flip_batch(256) != flip_batch(128)
    _check_forward('H256', 'euler')


def test_diffusion_net_shards_reproduce_the_whole_solve_bitwise():
    """H = 64, two-layer diffusion net, Euler: 8192 rows on 16-row tiles, 1024-row shards on the wave pairs unless planned globally."""
    assert path(net_model(), 8192) == 'mfma16' and path(net_model(), 1024) == 'w4'
    _check_forward('net', 'euler')


def _flat_grad(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double()


def _backward(name, spans, weights, **options):
    m = _problem(name)[0]
    m.requires_grad_(True)
    m.zero_grad(set_to_none=True)
    try:
        gy = []
        for lo, hi in spans:
            ys, y0 = _solve(name, 'euler', lo, hi, grad=True, **options)
            (ys[-1] * weights[lo:hi]).sum().backward()
            gy.append(y0.grad)
        torch.cuda.synchronize()
        return torch.cat(gy), _flat_grad(m)
    finally:
        m.zero_grad(set_to_none=True)
        m.requires_grad_(False)


@pytest.mark.parametrize('name', ['H128', 'net'])
def test_shard_adjoints_are_bitwise_and_parameter_gradients_within_the_margin(name):
    """Loss = sum of the final states times a fixed random tensor.  dL/dy0 of the shards planned with global_rows equals the whole
    solve's rows bit for bit; the parameter gradient summed over the shards agrees within GRAD_TOL (another summation order)."""
    _, _, _, N = _problem(name)
    H = _case(name)[2]
    n = N // SHARDS
    w = torch.randn((N, H), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    spans = [(r * n, (r + 1) * n) for r in range(SHARDS)]
    gy, gp = _backward(name, [(0, N)], w)
    gy_g, gp_g = _backward(name, spans, w, global_rows=N)
    gy_l, _ = _backward(name, spans, w)
    assert bool(torch.isfinite(gy).all()) and bool(torch.isfinite(gp).all()) and float(gp.abs().max()) > 0
    assert torch.equal(gy_g, gy)
    assert not torch.equal(gy_l, gy)
    err = (gp_g - gp).abs()
    rel_max, rel_mean = float(err.max() / gp.abs().max()), float(err.mean() / gp.abs().mean())
    print(f'{name}: flat parameter gradient, shards against whole: max-rel {rel_max:.2e} mean-rel {rel_mean:.2e}')
    assert rel_max < GRAD_TOL and rel_mean < GRAD_TOL, (rel_max, rel_mean)


def test_a_shard_the_global_plans_kernel_cannot_run_raises_and_launches_nothing(monkeypatch):
    """Two rows of a 1024-row problem planned onto the wave pairs (a tile is four rows): UNSUPPORTED, with or without `strict`,
    with or without gradients - never the generic kernels or the tensor loop in the wave pairs' place."""
    launched = []
    monkeypatch.setattr(engine.SolveCall, 'launch', lambda self, *a, **k: launched.append(1))
    monkeypatch.setattr(S.torchsde, '_sdeint_torch', lambda *a, **k: launched.append(2))
    m, t, ts, _ = _problem('net')
    m.set_X(t['coeffs'][:2].contiguous(), t['times'])
    y0 = t['y0'][:2].clone()
    assert path(net_model(), 2, global_rows=1024) == 'none' and path(net_model(), 2) != 'none'
    for strict in (True, False):
        with torch.no_grad():
            with pytest.raises(engine._lib.SnsdeError) as exc:
                S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'global_rows': 1024, 'strict': strict})
        assert exc.value.code == -4                      # SNSDE_ERR_UNSUPPORTED
        with pytest.raises(engine._lib.SnsdeError) as exc:
            S.sdeint(m, y0.clone().requires_grad_(True), ts, dt=1.0, method='euler', options={'global_rows': 1024, 'strict': strict})
        assert exc.value.code == -4
    assert not launched
    monkeypatch.undo()
    # the library itself refuses the launch (the check above is the Python layer's)
    grid = engine.step_grid(ts.cpu().numpy(), 1.0, t['times'].cpu().numpy(), torch.device(DEV))
    flat = engine.flatten_params(m, *engine.recognise(m)[1:], torch.device(DEV))
    call = engine.SolveCall(net_model(), flat, t['coeffs'][:2].contiguous(), grid, y0, global_rows=1024)
    with pytest.raises(engine._lib.SnsdeError) as exc:
        call.launch()
    assert exc.value.code == -4


def test_captured_graph_replays_match_eager_solves_with_global_rows():
    m, t, ts, N = _problem('H128')
    n = N // SHARDS
    lo = 3 * n
    m.set_X(t['coeffs'][lo:lo + n].contiguous(), t['times'])
    y0 = t['y0'][lo:lo + n].clone()
    opts = {'global_rows': N, 'row_offset': lo}
    state = S.torchsde.prepare_graph_capture(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options=dict(opts, seed=1))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static = S.sdeint(m, y0, ts, dt=1.0, method='euler', options=opts)
        outs = []
        for key in (1234567, 987654321):
            state.fill_(key - 1)           # the recorded solve advances the key by one, then reads it
            g.replay()
            outs.append(static.clone())
        eager = [S.sdeint(m, y0, ts, dt=1.0, method='euler', options=dict(opts, seed=k)) for k in (1234567, 987654321)]
        local = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'row_offset': lo, 'seed': 1234567})
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1])
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], local)
