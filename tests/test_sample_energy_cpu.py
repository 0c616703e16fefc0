"""The energy score of sample paths on the host: the entry points snsde_sample_energy / _backward (declared, exported, bound,
validating before they launch), and sample_energy / energy_loss on CPU tensors - the tensor-op statement of the definition -
against hand-written answers, the CRPS at width 1, and brute-force float64 over the (N, N, V) differences.  No GPU compute."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine, train

ERR_NULL, ERR_DIMS = -1, -2
NAMES = ('snsde_sample_energy', 'snsde_sample_energy_backward')


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (11, 13)):
        assert f'SNSDE_API int {name}(' in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f' T {name}\n' in dyn
        assert len(getattr(lib, name).argtypes) == arity
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)
    assert S.sample_energy is engine.sample_energy and S.energy_loss is train.energy_loss


def _fwd(lib, outer=1, members=1, groups=1, samples=4, width=1, fair=1, path=0, ys=4096, target=4096, energy=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_energy(p(ys), p(target), outer, members, groups, samples, width, fair, path, p(energy), None)


def _bwd(lib, outer=1, members=1, groups=1, samples=4, width=1, fair=1, path=0, g=4096, ys=4096, target=4096, gys=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_energy_backward(p(g), p(ys), p(target), outer, members, groups, samples, width, fair, path, p(gys), None, None)


def test_the_entry_points_validate_before_they_launch():
    lib = _lib.lib()
    for fn in (_fwd, _bwd):
        for path in (0, 1):
            assert fn(lib, ys=0, path=path) == ERR_NULL and fn(lib, target=0, path=path) == ERR_NULL
            assert fn(lib, outer=0, path=path) == ERR_DIMS and fn(lib, members=0, path=path) == ERR_DIMS
            assert fn(lib, groups=0, path=path) == ERR_DIMS and fn(lib, samples=0, path=path) == ERR_DIMS
            assert fn(lib, width=0, path=path) == ERR_DIMS and fn(lib, groups=-3, path=path) == ERR_DIMS
            assert fn(lib, samples=257, path=path) == ERR_DIMS                                # N > 256
            assert fn(lib, samples=1, members=257, path=path) == ERR_DIMS
            assert fn(lib, samples=129, members=2, path=path) == ERR_DIMS                     # N = 258
            assert fn(lib, samples=1, members=1, fair=1, path=path) == ERR_DIMS               # the unbiased estimator of one sample
            assert fn(lib, groups=2 ** 62, width=8, path=path) == ERR_DIMS                    # 63-bit overflow
            assert fn(lib, outer=2 ** 40, groups=2 ** 20, width=64, path=path) == ERR_DIMS
    assert _fwd(lib, energy=0) == ERR_NULL
    assert _bwd(lib, g=0) == ERR_NULL and _bwd(lib, gys=0) == ERR_NULL


# ---- exact hand answers ---------------------------------------------------------------------------------------------------------------
# case 1: x = {(0,0), (3,4)}, y = (3,0): r = 3, 4, r_12 = 5: fair 7/2 - 5/2 = 1, unfair 7/2 - 5/4 = 2.25
# case 2: x = {(1,2), (1,2), (0,0)}, y = (0,0) - a duplicate, and a sample on the observation: r = sqrt5, sqrt5, 0;
#   r_12 = 0, r_13 = r_23 = sqrt5; fair: 2 sqrt5 / 3 - 2 sqrt5 / 6 = sqrt5 / 3
#   d/dx_1 = u(x_1 - y) / 3 - (u(0) + u(x_1 - x_3)) / 6 = (1,2)/sqrt5 (1/3 - 1/6) = (1,2) / (6 sqrt5), the same for x_2
#   d/dx_3 = u(0) / 3 - 2 u(x_3 - x_1) / 6 = (1,2) / (3 sqrt5) = (2,4) / (6 sqrt5)
#   d/dy   = -(2 (1,2)/sqrt5 + u(0)) / 3 = -(2,4) / (3 sqrt5)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_exact_hand_answers_with_a_duplicate_and_a_sample_on_the_observation(dtype):
    x = torch.tensor([[0., 0.], [3., 4.]], dtype=dtype)
    y = torch.tensor([[3., 0.]], dtype=dtype)
    e = S.sample_energy(x, 2, y)
    assert e.shape == (1,) and e.dtype == dtype and e.item() == 1.0
    assert S.sample_energy(x, 2, y, fair=False).item() == 2.25
    x = torch.tensor([[1., 2.], [1., 2.], [0., 0.]], dtype=dtype, requires_grad=True)
    y = torch.tensor([[0., 0.]], dtype=dtype, requires_grad=True)
    e = S.sample_energy(x, 3, y)
    eps = 4 * torch.finfo(dtype).eps
    s5 = math.sqrt(5.0)
    assert abs(e.item() - s5 / 3) <= eps
    e.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(y.grad).all())
    want_x = torch.tensor([[1., 2.], [1., 2.], [2., 4.]], dtype=torch.float64) / (6 * s5)
    want_y = -torch.tensor([[2., 4.]], dtype=torch.float64) / (3 * s5)
    assert float((x.grad.double() - want_x).abs().max()) <= eps and float((y.grad.double() - want_y).abs().max()) <= eps


def _brute64(x, y, fair):
    """float64 over the (G, N, N, V) differences: mean_n ||x_n - y|| - sum_{n,j} ||x_n - x_j|| / (2 N D); x (G, N, V), y (G, V)."""
    N = x.shape[1]
    D = N - 1 if fair else N
    a = (x - y[:, None]).square().sum(-1).sqrt().sum(1) / N
    d2 = (x[:, :, None] - x[:, None, :]).square().sum(-1)
    b = torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt().where(d2 > 0, torch.zeros_like(d2)).sum((1, 2)) / (2 * N * D)
    return a - b


@pytest.mark.parametrize('fair', [True, False])
def test_random_inputs_against_brute_force_float64(fair):
    G, Sn, W = 5, 7, 3
    gen = torch.Generator().manual_seed(21)
    x32, y32 = torch.randn(G * Sn, W, generator=gen), torch.randn(G, W, generator=gen)
    x64, y64 = x32.double().requires_grad_(True), y32.double().requires_grad_(True)
    ref = _brute64(x64.reshape(G, Sn, W), y64, fair)
    gx_ref, gy_ref = torch.autograd.grad(ref.sum(), (x64, y64))
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 1e-5)):
        x, y = x32.to(dtype).requires_grad_(True), y32.to(dtype).requires_grad_(True)
        e = S.sample_energy(x, Sn, y, fair=fair)
        assert e.shape == (G,) and e.dtype == dtype
        assert float((e.detach().double() - ref.detach()).abs().max()) <= tol
        gx, gy = torch.autograd.grad(e.sum(), (x, y))
        assert float((gx.double() - gx_ref).abs().max()) <= tol and float((gy.double() - gy_ref).abs().max()) <= tol
    stacked = S.sample_energy(torch.stack([x32, 2 * x32]), Sn, torch.stack([y32, 2 * y32]), fair=fair)      # leading axes
    assert stacked.shape == (2, G) and torch.equal(stacked[0], S.sample_energy(x32, Sn, y32, fair=fair))


def test_width_one_is_the_crps():
    G, Sn = 6, 9
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(3, G * Sn, 1, generator=gen, dtype=torch.float64)
    x[:, 1] = x[:, 0]
    y = torch.randn(3, G, 1, generator=gen, dtype=torch.float64)
    for fair in (True, False):
        e, c = S.sample_energy(x, Sn, y, fair=fair), S.sample_crps(x, Sn, y, fair=fair)[..., 0]
        assert e.shape == c.shape == (3, G) and float((e - c).abs().max()) <= 1e-12


def test_path_mode_is_the_call_on_the_flattened_leading_axes():
    T_, G, Sn, W = 4, 3, 5, 2
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(T_, G * Sn, W, generator=gen, dtype=torch.float64, requires_grad=True)
    y = torch.randn(T_, G, W, generator=gen, dtype=torch.float64, requires_grad=True)
    e = S.sample_energy(x, Sn, y, path=True)
    flat_x = x.movedim(0, -2).reshape(G * Sn, T_ * W)
    flat_y = y.movedim(0, -2).reshape(G, T_ * W)
    ref = S.sample_energy(flat_x, Sn, flat_y)
    assert e.shape == (G,) and float((e - ref).detach().abs().max()) <= 1e-13
    ga, gb = torch.autograd.grad(e.sum(), (x, y)), torch.autograd.grad(ref.sum(), (x, y))
    assert float((ga[0] - gb[0]).abs().max()) <= 1e-13 and float((ga[1] - gb[1]).abs().max()) <= 1e-13
    assert float((e - _brute64(flat_x.reshape(G, Sn, T_ * W), flat_y, True)).detach().abs().max()) <= 1e-13
    # two leading axes, and members: everything in front of (members, rows, width) joins the vector
    x2 = torch.randn(2, 3, 2, G * Sn, W, generator=gen, dtype=torch.float64)
    y2 = torch.randn(2, 3, G, W, generator=gen, dtype=torch.float64)
    e2 = S.sample_energy(x2, Sn, y2, members=2, path=True)
    pooled = x2.reshape(6, 2, G, Sn, W).permute(2, 1, 3, 0, 4).reshape(G * 2 * Sn, 6 * W)
    assert e2.shape == (G,) and float((e2 - S.sample_energy(pooled, 2 * Sn, y2.reshape(6, G, W).movedim(0, -2).reshape(G, 6 * W))).abs().max()) <= 1e-13


def test_pooled_members_equal_the_hand_pooled_tensor():
    O, M, G, Sn, W = 2, 3, 2, 4, 5
    gen = torch.Generator().manual_seed(24)
    x = torch.randn(O, M, G * Sn, W, generator=gen)
    x[0, 1, 2] = x[0, 0, 1]      # (coincident samples across members)
    y = torch.randn(O, G, W, generator=gen)
    flat = x.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W).contiguous()
    for fair in (True, False):
        a, b = S.sample_energy(x, Sn, y, fair=fair, members=M), S.sample_energy(flat, M * Sn, y, fair=fair)
        assert a.shape == (O, G) and torch.equal(a, b)
    xa, xb = x.clone().requires_grad_(True), flat.clone().requires_grad_(True)
    S.sample_energy(xa, Sn, y, members=M).sum().backward()
    S.sample_energy(xb, M * Sn, y).sum().backward()
    assert bool(torch.isfinite(xa.grad).all())
    assert torch.equal(xa.grad.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), xb.grad)


def test_the_tensor_op_statement_slices_its_distance_plane_without_changing_a_value(monkeypatch):
    G, Sn, W = 7, 5, 3
    gen = torch.Generator().manual_seed(26)
    x, y = torch.randn(2, G * Sn, W, generator=gen), torch.randn(2, G, W, generator=gen)
    whole = engine.sample_energy_tensor_ops(x, Sn, y)
    monkeypatch.setattr(engine, '_CDIST_MAX_PLANE', 3 * Sn * Sn)      # three groups per torch.cdist call: 14 groups in five slices
    xs = x.clone().requires_grad_(True)
    sliced = engine.sample_energy_tensor_ops(xs, Sn, y)
    assert sliced.shape == (2, G) and torch.equal(sliced.detach(), whole)
    sliced.sum().backward()
    assert bool(torch.isfinite(xs.grad).all()) and float(xs.grad.abs().min()) > 0


def test_shape_errors_are_value_errors():
    x, y = torch.zeros(12, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match='whole number'):
        S.sample_energy(x, 5, y)
    with pytest.raises(ValueError, match='target'):
        S.sample_energy(x, 3, torch.zeros(4))
    with pytest.raises(ValueError, match='target'):
        S.sample_energy(x, 3, torch.zeros(3, 3), path=True)
    with pytest.raises(ValueError, match='at least 2'):
        S.sample_energy(x, 1, torch.zeros(12, 3))
    assert float((S.sample_energy(x, 1, torch.ones(12, 3), fair=False) - math.sqrt(3.0)).abs().max()) < 1e-6      # N = 1: ||x - y||
    with pytest.raises(ValueError, match='members'):
        S.sample_energy(x, 3, y, members=0)
    with pytest.raises(ValueError, match='samples'):
        S.sample_energy(x, 0, y)
    assert S.sample_energy(torch.zeros(0, 3), 2, torch.zeros(0, 3)).shape == (0,)
    assert S.sample_energy(torch.zeros(0, 4, 3), 2, torch.zeros(0, 2, 3), path=True).shape == (2,)


def test_energy_loss_on_forecasting_shaped_predictions():
    B, Sn, T_out, Cn = 3, 4, 5, 2
    gen = torch.Generator().manual_seed(25)
    pred = torch.randn(B * Sn, T_out, Cn, generator=gen, requires_grad=True)
    true = torch.randn(B, T_out, Cn, generator=gen)
    loss = S.energy_loss(Sn)(pred, true)
    want = _brute64(pred.detach().double().reshape(B, Sn, T_out * Cn), true.double().reshape(B, T_out * Cn), True).mean()
    assert loss.shape == () and abs(loss.item() - want.item()) <= 1e-5      # the whole forecast path is one vector
    assert torch.equal(loss, S.sample_energy(pred.reshape(B * Sn, T_out * Cn), Sn, true.reshape(B, T_out * Cn)).mean())
    loss.backward()
    assert pred.grad.shape == pred.shape and float(pred.grad.abs().sum()) > 0
    assert torch.equal(S.energy_loss(Sn, fair=False)(pred, true),
                       S.sample_energy(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), fair=False).mean())
    with pytest.raises(ValueError, match='energy_loss'):
        S.energy_loss(Sn)(pred[:-1], true)
    with pytest.raises(ValueError, match='energy_loss'):
        S.energy_loss(Sn)(pred, true[:-1])
    M = 2
    pm = torch.randn(M, B * Sn, T_out, Cn, generator=gen)      # an Ensemble's (M, B S, ...) output: the members' paths are pooled
    assert torch.equal(S.energy_loss(Sn, members=M)(pm, true),
                       S.sample_energy(pm.reshape(M, B * Sn, -1), Sn, true.reshape(B, -1), members=M).mean())
    with pytest.raises(ValueError, match='energy_loss'):
        S.energy_loss(Sn, members=3)(pm, true)
    with pytest.raises(ValueError, match='samples'):
        S.energy_loss(0)


def test_a_train_loop_epoch_on_the_cpu_trains_on_the_energy_loss():
    torch.manual_seed(3)
    n, L, Cn, H, Sn = 8, 5, 2, 4, 3
    rng = np.random.default_rng(5)
    times = np.arange(L, dtype=np.float32)
    slope = rng.standard_normal((n, 1, Cn)).astype(np.float32) * 0.2
    X = slope * times[None, :, None] + 0.05 * rng.standard_normal((n, L, Cn)).astype(np.float32)
    X[:, :, 0] = times[None]
    y = torch.from_numpy(np.stack([slope[:, 0, 1], -slope[:, 0, 1]], 1).astype(np.float32))
    coeffs = torch.cat(S.controldiffeq.natural_cubic_spline_coeffs(torch.from_numpy(times), torch.from_numpy(X)), dim=-1)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(coeffs, y, torch.full((n,), L - 1, dtype=torch.int64)), batch_size=n)
    model, field = S.make_sde_model('neurallsde', Cn, 2, H, H, 1)
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    kwargs = dict(method='euler', options={'seed': 1, 'samples': Sn, 'sample_grad': True})
    hist = train.train_loop(loader, loader, model, torch.from_numpy(times), opt, S.energy_loss(Sn), 1, None, 'cpu', kwargs, 'valloss')
    assert len(hist) == 1 and np.isfinite(hist[0].train_metrics.loss) and hist[0].train_metrics.loss > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
