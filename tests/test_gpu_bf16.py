"""bf16 MFMA operands on the GPU (options={'precision': 'bf16'}, SNSDE_FLAG_BF16_OPERANDS, csrc/snsde_m4b_kernel.h): the route,
the states against the numpy reference with the same operand rounding (tests/bf16_reference.py), bit-identity of everything
outside the operands, the accuracy against the f32 kernel at K2, the refusals and a captured graph."""
import signal
import zlib

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.bf16_reference import solve_bf16
from tests.helpers import draw_dW, make_problem, param_spec

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """every test of this file under its own time limit"""
    def fire(*_):
        raise TimeoutError('bf16 GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(300)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class _ReplayBM:
    def __init__(self, dW):
        self.dW, self.n = dW, 0

    def __call__(self, ta, tb):
        i, self.n = self.n, self.n + 1
        return self.dW[i]


def _field(pr, grad=False):
    m = S.Diffusion_model(pr['C'], pr['H'], pr['H'], pr['NL'], input_option=pr['io'], noise_option=pr['no'])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(DEV).requires_grad_(grad)
    times = torch.from_numpy(pr['times']).to(DEV)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), times)
    return m, times


def _k2_call(rows=1024, precision='fp32', seed=2024, zero_weights=False, dW=None):
    import bench
    pr, p0, flat, coeffs, y0 = bench.build_inputs(torch.device(DEV), 0, b=rows)
    if zero_weights:
        p0 = {k: (np.zeros_like(v) if k.endswith('weight') and not k.startswith('noise') else v) for k, v in p0.items()}
        flat = torch.from_numpy(np.concatenate([p0[n].reshape(-1) for n, _ in param_spec(4, 17, 2, 21, 128)])).to(DEV)
    model = engine.model_struct(21, 128, 128, 2, 4, 17)
    grid = engine.step_grid(np.array([0.0, 100.0], np.float32), 1.0, pr['times'], torch.device(DEV))
    return engine.SolveCall(model, flat, coeffs, grid, y0, dW=dW, seed=seed, precision=precision), pr, grid


def test_k2_routes_to_the_bf16_kernel_and_sdeint_runs_it():
    """K2 at 1024 rows: the host query names the bf16 kernel, and sdeint(options={'precision': 'bf16'}) returns what that
    kernel returns (bit for bit, same Philox key), not the f32 kernel's states."""
    model = engine.model_struct(21, 128, 128, 2, 4, 17)
    assert engine.forward_path(model, 1024, 101, 100, precision='bf16') == 'lean-bf16'
    call16, pr, grid = _k2_call(precision='bf16', seed=77)
    call32, _, _ = _k2_call(precision='fp32', seed=77)
    ys16, ys32 = call16.launch().clone(), call32.launch().clone()
    m, _ = _field(pr)
    with torch.no_grad():
        got = S.sdeint(m, torch.from_numpy(pr['y0']).to(DEV), torch.tensor([0.0, 100.0], device=DEV), dt=1.0, method='euler',
                       options={'precision': 'bf16', 'seed': 77})
    torch.cuda.synchronize()
    assert torch.equal(got, ys16)
    assert not torch.equal(ys16, ys32)
    assert float((ys16 - ys32).norm() / ys32.norm()) < 2e-2


# (io, no, NL, B, H, C, L, method): K2-shaped and small fuzzed cases over the covered options
CASES = [(4, 17, 2, 64, 128, 21, 16, 'euler'), (4, 17, 2, 64, 128, 21, 16, 'milstein')]
_rng = np.random.default_rng(2026)
for _H in (64, 128):
    for _NL in (1, 2, 3):
        for _ in range(3):
            _io = int(_rng.integers(0, 7))
            _no = int(_rng.choice([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 16, 17]))
            _m = str(_rng.choice(['euler', 'milstein']))
            CASES.append((_io, _no, _NL, int(_rng.integers(5, 40)), _H, int(_rng.integers(2, 30)), int(_rng.integers(5, 12)), _m))


def _covered(c):
    io, no, NL, B, H, C, L, method = c
    return engine.forward_path(engine.model_struct(C, H, H, NL, io, no), B, L, L - 1, method, precision='bf16') == 'lean-bf16'


def test_fuzz_list_spans_the_covered_options():
    cov = [c for c in CASES if _covered(c)]
    assert {c[4] for c in cov} == {64, 128} and {c[2] for c in cov} == {1, 2, 3}
    assert {c[7] for c in cov} == {'euler', 'milstein'} and len({c[0] for c in cov}) >= 5 and len(cov) >= 12


@pytest.mark.parametrize('case', [c for c in CASES if _covered(c)], ids=lambda c: '-'.join(map(str, c)))
def test_states_match_the_bf16_reference(case):
    """Supplied increments; ys against the fp64 restatement with the same operand rounding.  The states agree to the f32
    accumulation order, except where an operand lies within f32 round-off of a bf16 rounding boundary and the two sides round
    it to neighbouring bf16 values (one bf16 ulp = 2^-8 relative in ONE product).  Bounds: relative L2 1e-4, and max abs 1e-3
    per unit of the largest state: the multiplicative diffusions (no = 17 among them) let K2-shaped states grow to |y| ~ 5 within
    15 steps and carry such a flip along with them (measured there: relative L2 3.8e-5, max abs 1.4e-3; the fuzzed cases stay
    below 1e-3 absolute)."""
    io, no, NL, B, H, C, L, method = case
    pr = make_problem(zlib.crc32(repr(case).encode()) & 0xFFFF, io, no, NL, B, H, C, L)
    ts = pr['times']
    dW = draw_dW(5, ts, 1.0, B, H)
    m, times = _field(pr)
    with torch.no_grad():
        ys = S.sdeint(m, torch.from_numpy(pr['y0']).to(DEV), times, dt=1.0, method=method,
                      bm=_ReplayBM(torch.from_numpy(dW).to(DEV)), options={'precision': 'bf16'})
    ref, _ = solve_bf16(pr['params'], io, no, pr['coeffs'], pr['times'], pr['y0'], ts, 1.0, dW, method=method)
    got = ys.double().cpu().numpy()
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert rel <= 1e-4 and np.abs(got - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max()), (rel, np.abs(got - ref).max())


def test_zero_weights_bf16_equals_fp32_bitwise():
    """Every weight matrix of the drift MLP zero (biases, theta and the diffusion MLP kept): the operands are gone, what is left -
    diffusion, increments, update, interpolation - must be the f32 kernel's to the bit, with Philox and with supplied dW."""
    a, _, grid = _k2_call(precision='bf16', seed=5, zero_weights=True)
    b, _, _ = _k2_call(precision='fp32', seed=5, zero_weights=True)
    assert torch.equal(a.launch(), b.launch())
    dW = torch.from_numpy(draw_dW(9, np.array([0.0, 100.0], np.float32), 1.0, 1024, 128)).to(DEV)
    a, _, _ = _k2_call(precision='bf16', zero_weights=True, dW=dW)
    b, _, _ = _k2_call(precision='fp32', zero_weights=True, dW=dW)
    ya, yb = a.launch(), b.launch()
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and float(ya.abs().max()) > 0


def test_k2_accuracy_against_fp32():
    """K2 (1024 x 128, 100 Euler steps, Philox key 2024): bf16 operands against the f32 kernel.  Measured on MI355X:
    relative L2 4.12e-3 and max abs 3.49 over all outputs (the multiplicative diffusion lets states reach |y| ~ 75 by t = 100,
    and carries the operand rounding along); the bounds below are 2x those.  A fixed linear readout (10 classes) of the final
    states picks the same argmax for 1023 of the 1024 rows (0.9990)."""
    a, _, _ = _k2_call(precision='bf16')
    b, _, _ = _k2_call(precision='fp32')
    ya, yb = a.launch().double(), b.launch().double()
    rel = float((ya - yb).norm() / yb.norm())
    mx = float((ya - yb).abs().max())
    W = torch.from_numpy(np.random.default_rng(1).standard_normal((128, 10))).to(DEV)
    agree = float((ya[-1] @ W).argmax(1).eq((yb[-1] @ W).argmax(1)).double().mean())
    print(f'K2 bf16 vs fp32: relative L2 {rel:.3e}, max abs {mx:.3e}, readout argmax agreement {agree:.4f}')
    assert rel <= REL_BOUND and mx <= MAX_BOUND and agree >= AGREE_BOUND, (rel, mx, agree)


REL_BOUND, MAX_BOUND, AGREE_BOUND = 8.3e-3, 7.0, 0.99


def test_unsupported_requests_raise_and_launch_nothing(monkeypatch):
    launched = []
    monkeypatch.setattr(engine.SolveCall, 'launch', lambda self, *a, **k: launched.append(1))
    pr = make_problem(3, 4, 17, 2, 16, 64, 5, 6)
    m, times = _field(pr)
    y0 = torch.from_numpy(pr['y0']).to(DEV)
    with torch.no_grad():
        with pytest.raises(ValueError):
            S.sdeint(m, y0, times, dt=1.0, method='srk', options={'precision': 'bf16'})
    with pytest.raises(ValueError):
        S.sdeint(m, y0.clone().requires_grad_(True), times, dt=1.0, method='euler', options={'precision': 'bf16'})
    m.requires_grad_(True)
    with pytest.raises(ValueError):
        S.sdeint(m, y0, times, dt=1.0, method='euler', options={'precision': 'bf16'})
    pr = make_problem(3, 4, 17, 2, 16, 256, 5, 6)
    m, times = _field(pr)
    with torch.no_grad():
        with pytest.raises(ValueError):
            S.sdeint(m, torch.from_numpy(pr['y0']).to(DEV), times, dt=1.0, method='euler', options={'precision': 'bf16'})
        with pytest.raises(ValueError):       # training outputs
            S.sdeint(m, torch.from_numpy(pr['y0']).to(DEV), times, dt=1.0, options={'precision': 'bf16', 'save_traj': True})
    assert not launched


def test_captured_graph_replays_match_eager_bf16_solves():
    pr = make_problem(21, 4, 17, 2, 96, 128, 21, 12)
    m, times = _field(pr)
    y0 = torch.from_numpy(pr['y0']).to(DEV)
    state = S.torchsde.prepare_graph_capture(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            S.sdeint(m, y0, times, dt=0.5, method='euler', options={'precision': 'bf16', 'seed': 1})
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static = S.sdeint(m, y0, times, dt=0.5, method='euler', options={'precision': 'bf16'})
        outs = []
        for key in (1234567, 987654321):
            state.fill_(key - 1)           # the recorded solve advances the key by one, then reads it
            g.replay()
            outs.append(static.clone())
        eager = [S.sdeint(m, y0, times, dt=0.5, method='euler', options={'precision': 'bf16', 'seed': k}) for k in (1234567, 987654321)]
        f32 = S.sdeint(m, y0, times, dt=0.5, method='euler', options={'seed': 1234567})
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1])
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], f32)
