"""dL/dX of the spline coefficient constructions on the GPU: the two HIP adjoint kernels (snsde_natural_cubic_coeffs_backward,
snsde_hermite_coeffs_backward), the autograd node that carries them, and the routing of the public constructors.

Reference: torch.autograd through the package's tensor-op constructions in float64 on the CPU (tests/spline_grad_reference.py;
tests/test_spline_grad_cpu.py pins it against a restatement of the transposes).

Bound of the kernel comparison.  The kernel and the float32 tensor-op route are two float32 evaluations of the same linear map
in different operation orders.  The float32 route's own error against float64, e32(case) = max |g32 - g64| / max |g64|, is
computed here on the CPU for the same cases; the kernel is allowed 4 x the largest e32 of its kind over the cases, a small
factor for the reordering.  Measured on an MI355X host (profiles/spline_grad_margins.txt): the kernels sit below e32 itself.

Cases (tests/spline_grad_reference.py): irregular knots, L = 9 / 2 / 3; (B, C) = (3, 5) and (7, 21) - 147 series, a full
workgroup and a ragged second one; planted NaN patterns (none, interior gaps, either end or both missing, one observation,
two observations, none) in both workgroups, 30 % random NaN elsewhere; a standard-normal cotangent."""
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests import spline_grad_reference as R
from tests.helpers import grad_close
from tests.test_gpu_coeff_grad import GRAD_TOL_MAX

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
BOUND_FACTOR = 4.0
IDS = dict(ids=lambda k: 'L%d-B%d-C%d' % k)


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('spline-gradient GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(60)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _rel(a, ref):
    return float((a.double().cpu() - ref).abs().max()) / float(ref.abs().max())


_BOUND = {}


def _bound(kind):
    """4 x the float32 tensor-op route's own error against float64 (CPU), the largest over the cases."""
    if kind not in _BOUND:
        e32 = max(_rel(R.autograd_gradient(kind, key, torch.float32), R.autograd_gradient(kind, key)) for key in R.CASE_KEYS)
        assert 0 < e32 < 1e-4, e32
        _BOUND[kind] = (e32, BOUND_FACTOR * e32)
        print(f'{kind}: float32 tensor-op route vs float64 {e32:.3e}, bound {_BOUND[kind][1]:.3e}')
    return _BOUND[kind][1]


def _dev(c):
    return (torch.from_numpy(c['times']).float().to(DEV), torch.from_numpy(c['X']).float().to(DEV),
            torch.from_numpy(c['g']).float().to(DEV))


_KERNEL = {}


def _kernel(kind, key):
    if (kind, key) not in _KERNEL:
        _KERNEL[(kind, key)] = engine.spline_coeffs_backward(*_dev(R.case(*key)), kind)
        torch.cuda.synchronize()
    return _KERNEL[(kind, key)]


def _construct(kind, t, X):
    return R.tensor_op_coeffs(kind, t, X)      # the public constructors; the name says which route CPU tensors take


def _native_node(out):
    """True when the autograd graph of `out` holds the node of engine._SplineCoeffs (the HIP adjoint)."""
    seen, todo = set(), [out.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if '_SplineCoeffs' in type(n).__name__:
            return True
        todo.extend(f for f, _ in n.next_functions)
    return False


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------

@pytest.mark.parametrize('key', R.CASE_KEYS, **IDS)
@pytest.mark.parametrize('kind', R.KINDS)
def test_kernel_against_float64_autograd(kind, key):
    c = R.case(*key)
    ref = R.autograd_gradient(kind, key)
    got = _kernel(kind, key)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(c['X'].shape)
    assert bool(torch.isfinite(got).all())
    bound = _bound(kind)
    err = _rel(got, ref)
    print(f'{kind} {key}: kernel vs float64 autograd {err:.3e} (bound {bound:.3e})')
    gc = got.cpu().numpy()
    missing = np.isnan(c['X'])
    assert (gc[missing] == 0.0).all()                      # exact, no tolerance
    for (b, ch), name in c['planted'].items():
        if name == 'no observation':
            assert (gc[b, :, ch] == 0.0).all(), (b, ch)
    assert err < bound, (err, bound)


# ---- 2. same forward bits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', R.KINDS)
def test_forward_bits_do_not_depend_on_requires_grad(kind):
    t, X, _ = _dev(R.case(9, 7, 21))
    plain = _construct(kind, t, X.detach())
    tracked = _construct(kind, t, X.clone().requires_grad_(True))
    assert not plain.requires_grad and tracked.requires_grad
    assert _native_node(tracked)
    assert torch.equal(plain, tracked.detach())
    assert torch.equal(engine.spline_coeffs(t, X, kind), engine.spline_coeffs(t, X.clone().requires_grad_(True), kind).detach())


# ---- 3. determinism and row independence ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', R.KINDS)
def test_two_calls_and_a_row_slice_are_bit_equal(kind):
    key = (9, 7, 21)
    t, X, g = _dev(R.case(*key))
    whole = _kernel(kind, key)
    assert torch.equal(engine.spline_coeffs_backward(t, X, g, kind), whole)
    part = engine.spline_coeffs_backward(t, X[2:5].contiguous(), g[2:5].contiguous(), kind)
    assert torch.equal(part, whole[2:5])


# ---- 4. routing through the public constructors ---------------------------------------------------------------------------------

@pytest.mark.parametrize('key', [(9, 7, 21), (2, 3, 5)], **IDS)
@pytest.mark.parametrize('kind', R.KINDS)
def test_constructors_route_a_cuda_float32_input_to_the_kernel(kind, key, monkeypatch):
    t, X, g = _dev(R.case(*key))
    monkeypatch.delenv('SNSDE_SPLINE_GRAD', raising=False)
    Xn = X.clone().requires_grad_(True)
    out = _construct(kind, t, Xn)
    assert _native_node(out)
    (out * g).sum().backward()
    assert torch.equal(Xn.grad, _kernel(kind, key))
    monkeypatch.setenv('SNSDE_SPLINE_GRAD', 'torch')
    Xt = X.clone().requires_grad_(True)
    out_t = _construct(kind, t, Xt)
    assert out_t.requires_grad and not _native_node(out_t)      # autograd through the tensor ops, not the same kernel again
    (out_t * g).sum().backward()
    err = float((Xt.grad - Xn.grad).abs().max()) / float(Xn.grad.abs().max())
    print(f'{kind} {key}: tensor-op route vs kernel {err:.3e}')
    assert err < _bound(kind)
    assert bool((Xt.grad[torch.isnan(X)] == 0).all())


@pytest.mark.parametrize('kind', R.KINDS)
def test_float64_and_cpu_inputs_keep_the_tensor_op_route(kind, monkeypatch):
    monkeypatch.delenv('SNSDE_SPLINE_GRAD', raising=False)
    key = (9, 3, 5)
    c = R.case(*key)
    ref = R.autograd_gradient(kind, key)
    for device, dtype, tol in ((DEV, torch.float64, 1e-12), ('cpu', torch.float32, _bound(kind)), ('cpu', torch.float64, 1e-12)):
        X = torch.from_numpy(c['X']).to(device=device, dtype=dtype).requires_grad_(True)
        out = _construct(kind, torch.from_numpy(c['times']).to(device=device, dtype=dtype), X)
        assert out.dtype == dtype and out.device.type == torch.device(device).type
        (out * torch.from_numpy(c['g']).to(device=device, dtype=dtype)).sum().backward()
        assert X.grad.dtype == dtype and _rel(X.grad, ref) <= tol, (device, dtype)


def test_an_input_without_grad_builds_no_node():
    t, X, _ = _dev(R.case(9, 3, 5))
    for kind in R.KINDS:
        out = _construct(kind, t, X)
        assert out.grad_fn is None and not out.requires_grad
        with torch.no_grad():
            assert _construct(kind, t, X.clone().requires_grad_(True)).grad_fn is None


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------

def _wrapper(dtype, device, X, times, fi):
    """X -> natural coefficients -> NeuralSDE(final_index) -> output; a diffusion-free field (noise_option 0: g = 0), so the CPU
    and the GPU run integrate the same path without shared increments (tests/test_gpu_coeff_grad.py section 8, natural)."""
    Cn, H = X.shape[-1], 32
    torch.manual_seed(5)
    func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=0)
    net = S.NeuralSDE(func, Cn, H, 2).eval().to(device=device, dtype=dtype)
    t = torch.from_numpy(times).to(device=device, dtype=dtype)
    coeffs = torch.cat(S.controldiffeq.natural_cubic_spline_coeffs(t, X.to(device=device, dtype=dtype)), dim=-1)
    return net(t, (coeffs,), fi.to(device), method='euler'), coeffs


def test_wrapper_carries_the_gradient_back_to_observations_with_gaps(monkeypatch):
    monkeypatch.delenv('SNSDE_SPLINE_GRAD', raising=False)
    B, Cn = 5, 3
    times = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0], np.float32)
    rng = np.random.default_rng(9)
    X0 = (rng.standard_normal((B, len(times), Cn)) * 0.3).cumsum(1).astype(np.float32)
    X0[rng.random(X0.shape) < 0.3] = np.nan
    X0[0, 0, 0] = X0[1, -1, 1] = np.nan
    X0[2, :, 2] = np.nan
    X0 = torch.from_numpy(X0)
    fi = torch.tensor([6, 3, 6, 2, 4])
    w = torch.from_numpy(rng.standard_normal((B, 2)).astype(np.float32))
    Xr = X0.double().requires_grad_(True)
    out_r, _ = _wrapper(torch.float64, 'cpu', Xr, times, fi)
    (out_r * w.double()).sum().backward()
    Xg = X0.clone().to(DEV).requires_grad_(True)
    out_g, coeffs_g = _wrapper(torch.float32, DEV, Xg, times, fi)
    assert coeffs_g.requires_grad
    (out_g * w.to(DEV)).sum().backward()
    assert Xg.grad is not None and bool(torch.isfinite(Xg.grad).all()) and float(Xg.grad.abs().max()) > 0
    assert bool((Xg.grad[torch.isnan(Xg.detach())] == 0).all())
    grad_close(Xg.grad, Xr.grad, 'X', GRAD_TOL_MAX, 'natural wrapper')


# ---- 6. hipGraph -----------------------------------------------------------------------------------------------------------------

def test_captured_hermite_chain_replays_to_the_eager_gradient(monkeypatch):
    monkeypatch.delenv('SNSDE_SPLINE_GRAD', raising=False)
    t, X, w = _dev(R.case(9, 7, 21))
    X = X.clone().requires_grad_(True)

    def step():
        coeffs = S.torchcde.hermite_cubic_coefficients_with_backward_differences(X, t)
        return torch.autograd.grad((coeffs * w).sum(), [X])

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for s in static:
        s.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert float(eager[0].abs().max()) > 0
    assert torch.equal(static[0], eager[0]) and torch.equal(eager[0], _kernel('hermite', (9, 7, 21)))
