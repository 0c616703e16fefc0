"""dL/d coeffs of the fused solve on the GPU (snsde_coeff_gradients, and the batched autograd pass of the generic adjoints)
against the fp64 tensor-op loop on the CPU over identical supplied increments.

The mathematics.  X(t) enters the drift's first rectified layer only, and linearly.  With delta_p[b, :] = dL/d(pre-activation
of that layer) at drift pass p (N passes for Euler / Milstein, the 3N drift stages for SRK; delta slot nhid + 1), evaluated
at time t_p on spline interval k_p at offset r_p (step_tab columns 5 / 4; SRK: the stage-table slot of the pass's drift
stage), and M (H x C) the matrix that maps X(t) into that pre-activation (emb.weight[:, H:] @ initial_network.weight for
input_option 2 / 4 / 6, initial_network.weight for 0; 1 / 3 / 5 do not read X: exactly zero), v_p = M^T delta_p and

    grad_coeffs[b, k, j C + c] = sum_{p : k_p = k} phi_j(r_p) v_p[b, c],      phi = (1, r, r^2 / 2, r^3 / 3)

for the blocks (a, b, two_c, three_d).  The diffusion never reads X; intervals no pass falls into get exactly 0.

Arbiter and bounds: the fp64 loop on the CPU (options={'backend': 'torch'}), a wsum-weighted sum loss, and the project's
gradient yardstick of tests/test_gpu_parity.py: max error / max |ref| < 1e-4 and mean error / mean |ref| < 1e-4, for
coeffs.grad as for dL/dy0 and every parameter gradient.

Shapes: irregular knots, ts = [0, 2.5, 6], dt = 0.5 (two passes share an interval) and 1.0; rows 3 / 5 / 9 (ragged 4-row tiles),
channels 3 / 21 / 69, hidden sizes 32 / 64 / 128, one and two hidden layers.  With these knots every interval holds an Euler
step time at dt = 0.5 and at dt = 1.0; the intervals without a pass are read from the step table of each case and asserted
exactly zero, and one case at dt = 2.0 (three of six intervals empty) makes that assertion bite."""
import signal
import warnings

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from stable_neural_sdes_amd import torchsde as T
from tests.helpers import grad_close, make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0], np.float32)
TS = np.array([0.0, 2.5, 6.0], np.float32)
GRAD_TOL_MAX = GRAD_TOL_MEAN = 1e-4      # (tests/test_gpu_parity.py)

# (io, no) -> (H, C, B, NL, dt): every size of the list above is met once
SHAPES = {(4, 17): (128, 21, 5, 2, 0.5), (2, 16): (32, 3, 3, 1, 1.0), (6, 17): (64, 69, 9, 2, 0.5), (0, 17): (64, 3, 5, 2, 1.0)}


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('coefficient-gradient GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class _ReplayBM:
    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb, return_U=False):
        out = self.dW[self.n]
        u = self.dU[self.n] if self.dU is not None else None
        self.n += 1
        return (out, u) if return_U else out


_CASES = {}


def _case(io, no, NL, B, H, C_, dt, method, seed=0):
    """Inputs, increments, loss weights and the fp64 CPU reference of one configuration: computed once, shared, never modified."""
    key = (io, no, NL, B, H, C_, dt, method, seed)
    if key in _CASES:
        return _CASES[key]
    sd = 500 + seed + 11 * io + no + H + C_ + B
    pr = make_problem(sd, io, no, NL, B, H, C_, len(TIMES), times=TIMES)
    grid = engine.StepGrid(TS, dt, TIMES, None)
    rng = np.random.default_rng(sd)
    hh = (grid.t1 - grid.t0).astype(np.float32).reshape(-1, 1, 1)
    dW = (rng.standard_normal((grid.N, B, H)).astype(np.float32) * np.sqrt(hh)).astype(np.float32)
    dU = None
    if method == 'srk':
        dU = (hh * (0.5 * dW + np.sqrt(hh / 12) * rng.standard_normal(dW.shape).astype(np.float32))).astype(np.float32)
    wsum = rng.standard_normal((len(TS), B, H)).astype(np.float32)
    c = dict(pr=pr, dW=dW, dU=dU, wsum=wsum, grid=grid, io=io, no=no, NL=NL, B=B, H=H, C=C_, dt=dt, method=method)
    m, y0, coeffs = _build(c, torch.float64, 'cpu')
    ys = S.sdeint(m, y0, torch.from_numpy(TS), bm=_ReplayBM(torch.from_numpy(dW).double(), None if dU is None else torch.from_numpy(dU).double()),
                  method=method, dt=dt, options={'backend': 'torch'})
    (ys * torch.from_numpy(wsum).double()).sum().backward()
    c['ref'] = dict(ys=ys.detach(), y0=y0.grad, coeffs=coeffs.grad, params={n: p.grad for n, p in m.named_parameters()})
    _CASES[key] = c
    return c


def _build(c, dtype, device, rows=None):
    pr = c['pr']
    rows = slice(None) if rows is None else rows
    m = S.Diffusion_model(c['C'], c['H'], c['H'], c['NL'], input_option=c['io'], noise_option=c['no'])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(device=device, dtype=dtype)
    coeffs = torch.from_numpy(pr['coeffs'][rows]).to(device=device, dtype=dtype).requires_grad_(True)
    m.set_X(coeffs, torch.from_numpy(pr['times']).to(device))
    y0 = torch.from_numpy(pr['y0'][rows]).to(device=device, dtype=dtype).requires_grad_(True)
    return m, y0, coeffs


def _gpu(c, options, rows=None, backward=True):
    rows_ = slice(None) if rows is None else rows
    m, y0, coeffs = _build(c, torch.float32, DEV, rows)
    dW = torch.from_numpy(c['dW'][:, rows_]).to(DEV).contiguous()
    dU = None if c['dU'] is None else torch.from_numpy(c['dU'][:, rows_]).to(DEV).contiguous()
    ys = S.sdeint(m, y0, torch.from_numpy(TS).to(DEV), bm=_ReplayBM(dW, dU), method=c['method'], dt=c['dt'], options=options)
    if backward:
        (ys * torch.from_numpy(c['wsum'][:, rows_]).to(DEV)).sum().backward()
    return m, y0, coeffs, ys


def _empty_intervals(c):
    """Intervals no drift pass falls into, from the solver's own tables."""
    grid = c['grid']
    if c['method'] == 'srk':
        tab = np.zeros((grid.N, 4, 8), np.float32)
        engine._lib.check(engine._lib.lib().snsde_grid_srk_build(grid.step_tab.ctypes.data, grid.N, grid._times32.ctypes.data,
                                                                 grid._times32.shape[0], tab.ctypes.data))
        hit = set(tab[:, (0, 3, 2), 4].copy().view(np.int32).reshape(-1).tolist())
    else:
        hit = set(grid.step_tab[:, 5].copy().view(np.int32).tolist())
    return [k for k in range(len(TIMES) - 1) if k not in hit]


def _compare(c, m, y0, coeffs, ys, tag):
    ref = c['ref']
    fscale = float(ref['ys'].abs().max()) + 1e-12
    assert float((ys.detach().double().cpu() - ref['ys']).abs().max()) / fscale < 2e-4, 'forward'
    assert coeffs.grad is not None, 'coeffs.grad is None'
    g = coeffs.grad
    assert g.dtype == coeffs.dtype and tuple(g.shape) == tuple(coeffs.shape) and bool(torch.isfinite(g).all())
    e = (g.double().cpu() - ref['coeffs']).abs()
    print(f"{tag}: coeffs max {float(e.max()) / float(ref['coeffs'].abs().max()):.3e} mean {float(e.mean()) / float(ref['coeffs'].abs().mean()):.3e}")
    for k in _empty_intervals(c):
        assert float(g[:, k].abs().max()) == 0.0 and float(ref['coeffs'][:, k].abs().max()) == 0.0, k
    grad_close(g, ref['coeffs'], 'coeffs', GRAD_TOL_MAX, tag)
    grad_close(y0.grad, ref['y0'], 'y0', GRAD_TOL_MAX, tag)
    for name, p in m.named_parameters():
        gref = ref['params'][name]
        if gref is None or float(gref.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6, name
            continue
        grad_close(p.grad, gref, name, GRAD_TOL_MAX, tag)


def _assert_native(ys, mode=1):
    """A green run is the fused node: the MFMA adjoint with delta planes (mode 1) or the generic adjoint (mode 2)."""
    node = ys.grad_fn
    assert type(node).__name__.startswith('_FusedSolve'), type(node).__name__
    assert node.mode == mode, node.mode
    if mode == 1:
        assert node.call.delta_slots > 0 and node.coeffs_dtype is not None


# ---- 1. mode 1, Euler / Milstein ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'milstein'])
@pytest.mark.parametrize('io,no', [(4, 17), (2, 16), (6, 17), (0, 17)])
@pytest.mark.parametrize('kernel', ['mfma4', 'mfma16'])
def test_mfma_adjoint_returns_the_coefficient_gradient(kernel, io, no, method):
    H, C_, B, NL, dt = SHAPES[(io, no)]
    c = _case(io, no, NL, B, H, C_, dt, method)
    model = engine.model_struct(C_, H, H, NL, io, no)
    assert engine.backward_mode(model, B, len(TIMES), engine.step_grid(TS, dt, TIMES, torch.device(DEV)), method, kernel) == 1
    m, y0, coeffs, ys = _gpu(c, {'kernel': kernel, 'strict': True}, backward=False)
    _assert_native(ys)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    _compare(c, m, y0, coeffs, ys, f'{kernel} ({io},{no}) {method}')


def test_intervals_without_a_pass_get_exact_zeros():
    """dt = 2: the Euler step times 0, 2, 4 fall into intervals 0, 2 and 4; intervals 1, 3 and 5 receive exactly zero."""
    c = _case(4, 17, 2, 5, 64, 3, 2.0, 'euler')
    assert _empty_intervals(c) == [1, 3, 5]
    m, y0, coeffs, ys = _gpu(c, {'kernel': 'mfma4', 'strict': True}, backward=False)
    _assert_native(ys)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    _compare(c, m, y0, coeffs, ys, 'dt=2')
    assert float(coeffs.grad[:, 0].abs().max()) > 0


# ---- 2. SRK: stage times straddle a knot, intervals are revisited in pass order ---------------------------------------------

@pytest.mark.parametrize('io,no', [(4, 17), (0, 17)])
def test_srk_on_the_mfma_path(io, no):
    H, C_, B, NL, _ = SHAPES[(io, no)]
    """The forward runs the MFMA SRK kernel in both cases.  (4, 17) has the MFMA adjoint (mode 1: the new kernel walks 3N passes
    whose intervals are not monotone); the y-free drift of input_option 0 has none under SRK - the library answers mode 2 at
    every hidden size and tile flavour - so its gradient comes from the batched autograd pass of the generic adjoint."""
    c = _case(io, no, NL, B, H, C_, 1.0, 'srk')      # stages at t0, t0 + 1, t0 + 1/2: t0 = 0 visits intervals 0, 1, 0
    model = engine.model_struct(C_, H, H, NL, io, no)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert engine.forward_path(model, B, len(TIMES), grid.N, 'srk', 'mfma4') == 'mfma-srk'
    mode = engine.backward_mode(model, B, len(TIMES), grid, 'srk', 'mfma4')
    assert mode == (1 if io == 4 else 2)
    m, y0, coeffs, ys = _gpu(c, {'kernel': 'mfma4', 'strict': True}, backward=False)
    _assert_native(ys, mode)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    _compare(c, m, y0, coeffs, ys, f'srk ({io},{no})')


# ---- 3. exact order -----------------------------------------------------------------------------------------------------------

def test_exact_order_first_layer():
    c = _case(4, 17, 2, 5, 64, 3, 0.5, 'euler')
    m, y0, coeffs, ys = _gpu(c, {'kernel': 'mfma4', 'strict': True, 'exact_order': True}, backward=False)
    _assert_native(ys)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    _compare(c, m, y0, coeffs, ys, 'exact order')


# ---- 4. the kernel against the library-GEMM pass ---------------------------------------------------------------------------

def test_kernel_equals_the_library_gemm_pass_on_the_same_planes():
    """param_pass='torch' forms dL/d coeffs from the same delta plane with tensor ops ((delta E_x) W, then index_add_); the
    kernel folds M = E_x W first.  Both fp32, only the association and the summation order differ: 1e-5 of max |ref|."""
    c = _case(4, 17, 2, 5, 128, 21, 0.5, 'euler')
    _, _, ck, _ = _gpu(c, {'kernel': 'mfma4', 'strict': True})
    _, _, ct, _ = _gpu(c, {'kernel': 'mfma4', 'strict': True, 'param_pass': 'torch'})
    err = float((ck.grad - ct.grad).abs().max()) / float(ct.grad.abs().max())
    print(f'kernel vs gemm pass: {err:.3e}')
    assert err < 1e-5, err


# ---- 5. determinism and shard invariance -----------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_two_runs_and_a_shard_are_bit_equal(method):
    c = _case(4, 17, 2, 8, 64, 21, 0.5, method)
    _, _, c1, _ = _gpu(c, {'kernel': 'mfma4', 'strict': True})
    _, _, c2, _ = _gpu(c, {'kernel': 'mfma4', 'strict': True})
    assert torch.equal(c1.grad, c2.grad)
    _, _, cs, ys = _gpu(c, {'kernel': 'mfma4', 'strict': True, 'row_offset': 4, 'global_rows': 8}, rows=slice(4, 8))
    assert torch.equal(cs.grad, c1.grad[4:8])


# ---- 6. mode 2 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_generic_adjoint_takes_it_from_the_batched_autograd_pass(method):
    c = _case(4, 17, 2, 5, 24, 3, 0.5, method)
    m, y0, coeffs, ys = _gpu(c, {'kernel': 'generic', 'strict': True}, backward=False)
    _assert_native(ys, mode=2)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    _compare(c, m, y0, coeffs, ys, f'generic {method}')


# ---- 7. the fallback rule ----------------------------------------------------------------------------------------------------

def test_wave_pair_adjoint_falls_back_with_one_warning_or_raises_when_strict():
    c = _case(1, 18, 2, 12, 64, 3, 0.5, 'euler')
    model = engine.model_struct(3, 64, 64, 2, 1, 18)
    grid = engine.step_grid(TS, 0.5, TIMES, torch.device(DEV))
    assert engine.forward_path(model, 12, len(TIMES), grid.N, 'euler') == 'w4' and engine.backward_mode(model, 12, len(TIMES), grid, 'euler') == 1
    with pytest.raises(NotImplementedError, match='coefficients'):
        _gpu(c, {'strict': True})
    T._UNFUSED_WARNED.clear()
    with pytest.warns(UserWarning, match='coefficients') as rec:
        m, y0, coeffs, ys = _gpu(c, {})
    assert len([w for w in rec if 'coefficients' in str(w.message)]) == 1
    assert not type(ys.grad_fn).__name__.startswith('_FusedSolve')
    # the drift of input_option 1 does not read X: the loop's gradient is zero (autograd: no path to the leaf)
    assert c['ref']['coeffs'] is None or float(c['ref']['coeffs'].abs().max()) == 0.0
    assert coeffs.grad is None or float(coeffs.grad.abs().max()) == 0.0
    grad_close(y0.grad, c['ref']['y0'], 'y0', GRAD_TOL_MAX, 'fallback')
    with warnings.catch_warnings():
        warnings.simplefilter('error')      # (the second solve of the configuration warns no more)
        _gpu(c, {})


def test_a_drift_that_does_not_read_x_gets_zeros_on_the_lean_kernel_without_a_warning():
    c = _case(1, 17, 2, 5, 64, 3, 0.5, 'euler')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m, y0, coeffs, ys = _gpu(c, {'strict': True}, backward=False)
        _assert_native(ys)
        (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    assert coeffs.grad is not None and tuple(coeffs.grad.shape) == tuple(coeffs.shape) and float(coeffs.grad.abs().max()) == 0.0
    grad_close(y0.grad, c['ref']['y0'], 'y0', GRAD_TOL_MAX, 'io 1')


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------

def _wrapper(dtype, device, X, fi, no=0):
    """X -> Hermite coefficients -> NeuralSDE(final_index) -> loss; a diffusion-free field (noise_option 0: g = 0), so the
    CPU and the GPU run integrate the same path without shared increments."""
    Cn, H = X.shape[-1], 32
    torch.manual_seed(5)
    func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=no)
    net = S.NeuralSDE(func, Cn, H, 2).eval().to(device=device, dtype=dtype)
    times = torch.from_numpy(TIMES).to(device=device, dtype=dtype if dtype == torch.float64 else torch.float32)
    Xd = X.to(device=device, dtype=dtype)
    coeffs = S.torchcde.hermite_cubic_coefficients_with_backward_differences(Xd, times)
    out = net(times, (coeffs,), fi.to(device), method='euler')      # (dt = the smallest knot gap, 0.5)
    return net, out, coeffs


def test_wrapper_carries_the_gradient_back_to_the_observations():
    B, Cn = 5, 3
    rng = np.random.default_rng(9)
    X0 = torch.from_numpy((rng.standard_normal((B, len(TIMES), Cn)) * 0.3).cumsum(1).astype(np.float32))
    fi = torch.tensor([6, 3, 6, 2, 4])
    w = torch.from_numpy(rng.standard_normal((B, 2)).astype(np.float32))
    Xr = X0.double().requires_grad_(True)
    net_r, out_r, _ = _wrapper(torch.float64, 'cpu', Xr, fi)
    (out_r * w.double()).sum().backward()
    Xg = X0.clone().to(DEV).requires_grad_(True)
    net_g, out_g, coeffs_g = _wrapper(torch.float32, DEV, Xg, fi)
    assert coeffs_g.requires_grad
    (out_g * w.to(DEV)).sum().backward()
    assert Xg.grad is not None and bool(torch.isfinite(Xg.grad).all()) and float(Xg.grad.abs().max()) > 0
    grad_close(Xg.grad, Xr.grad, 'X', GRAD_TOL_MAX, 'wrapper')
    # coefficients that do not require grad: the solve is the one it was - same outputs and parameter gradients from a tensor and
    # from its detached copy, and the node carries no coefficient input
    outs = []
    for Xn in (X0.to(DEV), X0.to(DEV).detach().clone()):
        net, out, coeffs = _wrapper(torch.float32, DEV, Xn, fi)
        assert not coeffs.requires_grad
        (out * w.to(DEV)).sum().backward()
        outs.append((out.detach(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert torch.equal(outs[0][0], out_g.detach())


# ---- 9. hipGraph ------------------------------------------------------------------------------------------------------------

def test_captured_forward_and_backward_replay_to_the_eager_gradient():
    c = _case(4, 17, 2, 5, 64, 21, 0.5, 'euler')
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    ts = torch.from_numpy(TS).to(DEV)
    wsum = torch.from_numpy(c['wsum']).to(DEV)
    m, y0, coeffs = _build(c, torch.float32, DEV)

    def step():
        ys = S.sdeint(m, y0, ts, method='euler', dt=0.5, options={'kernel': 'mfma4', 'strict': True, 'seed': seed})
        return torch.autograd.grad((ys * wsum).sum(), [coeffs, y0])

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    for t in static:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0].abs().max()) > 0
    assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])
