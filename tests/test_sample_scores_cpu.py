"""Scores of sample paths on the host: the four entry points snsde_sample_crps / _backward / snsde_sample_quantiles / _backward
(declared, exported, bound, validating before they launch), and sample_crps / sample_quantiles / crps_loss on CPU tensors - the
tensor-op statement of the definitions - against hand-written answers and brute-force float64.  No GPU compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine

ERR_NULL, ERR_DIMS = -1, -2
NAMES = ('snsde_sample_crps', 'snsde_sample_crps_backward', 'snsde_sample_quantiles', 'snsde_sample_quantiles_backward')
U = 2.0 ** -24


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (12, 12, 11, 12)):
        assert f'SNSDE_API int {name}(' in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f' T {name}\n' in dyn
        assert len(getattr(lib, name).argtypes) == arity
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)


def _crps(lib, outer=1, members=1, groups=1, samples=4, width=1, fair=1, ys=4096, target=4096, crps=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_crps(p(ys), p(target), outer, members, groups, samples, width, fair, p(crps), None, None, None)


def _crps_bwd(lib, outer=1, members=1, groups=1, samples=4, width=1, fair=1, g=4096, ys=4096, target=4096, gys=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_crps_backward(p(g), p(ys), p(target), outer, members, groups, samples, width, fair, p(gys), None, None)


def _quant(lib, ks, fracs, n_q=None, outer=1, members=1, groups=1, samples=4, width=1, backward=False, ys=4096, out=4096):
    n = len(ks) if n_q is None else n_q
    k, f = (C.c_int32 * max(len(ks), 1))(*ks), (C.c_float * max(len(fracs), 1))(*fracs)
    p = lambda v: C.c_void_p(v) if v else None
    if backward:
        return lib.snsde_sample_quantiles_backward(p(4096), p(ys), outer, members, groups, samples, width, n, k, f, p(out), None)
    return lib.snsde_sample_quantiles(p(ys), outer, members, groups, samples, width, n, k, f, p(out), None)


def test_the_entry_points_validate_before_they_launch():
    lib = _lib.lib()
    for fn in (_crps, _crps_bwd):
        assert fn(lib, ys=0) == ERR_NULL and fn(lib, target=0) == ERR_NULL
        assert fn(lib, outer=0) == ERR_DIMS and fn(lib, members=0) == ERR_DIMS and fn(lib, groups=0) == ERR_DIMS
        assert fn(lib, samples=0) == ERR_DIMS and fn(lib, width=0) == ERR_DIMS and fn(lib, groups=-3) == ERR_DIMS
        assert fn(lib, samples=257) == ERR_DIMS                                # N > 256
        assert fn(lib, samples=1, members=257) == ERR_DIMS
        assert fn(lib, samples=129, members=2) == ERR_DIMS                     # N = 258
        assert fn(lib, samples=1, members=1, fair=1) == ERR_DIMS               # the unbiased estimator of one sample
        assert fn(lib, groups=2 ** 62, width=8) == ERR_DIMS                    # 63-bit overflow
        assert fn(lib, outer=2 ** 40, groups=2 ** 20, width=64) == ERR_DIMS
    assert _crps(lib, crps=0) == ERR_NULL
    assert _crps_bwd(lib, g=0) == ERR_NULL and _crps_bwd(lib, gys=0) == ERR_NULL
    for backward in (False, True):
        q = lambda ks, fracs, **kw: _quant(lib, ks, fracs, backward=backward, **kw)
        assert q([0], [0.0], ys=0) == ERR_NULL and q([0], [0.0], out=0) == ERR_NULL
        assert q([0], [0.0], n_q=0) == ERR_DIMS and q([0] * 9, [0.0] * 9) == ERR_DIMS       # n_q outside 1 .. 8
        assert q([-1], [0.0]) == ERR_DIMS and q([4], [0.0]) == ERR_DIMS                     # k outside [0, N - 1]
        assert q([1], [1.0]) == ERR_DIMS and q([1], [-0.5]) == ERR_DIMS                     # frac outside [0, 1)
        assert q([1], [float('nan')]) == ERR_DIMS
        assert q([3], [0.25]) == ERR_DIMS                                                   # k = N - 1 with frac > 0
        assert q([0], [0.0], samples=257) == ERR_DIMS and q([0], [0.0], width=0) == ERR_DIMS
        assert q([0], [0.0], samples=129, members=2) == ERR_DIMS
    k = (C.c_int32 * 1)(0)
    f = (C.c_float * 1)(0.0)
    p = C.c_void_p(4096)
    assert lib.snsde_sample_quantiles(p, 1, 1, 1, 4, 1, 1, None, f, p, None) == ERR_NULL
    assert lib.snsde_sample_quantiles(p, 1, 1, 1, 4, 1, 1, k, None, p, None) == ERR_NULL
    assert lib.snsde_sample_quantiles_backward(None, p, 1, 1, 1, 4, 1, 1, k, f, p, None) == ERR_NULL


# ---- exact known answers: integer-valued inputs, N = 4, fair=False, every operation exact -------------------------------------------
# case 1, a duplicated sample: x = (1, 3, 3, 7), y = 4
#   d = (-3, -1, -1, 3), sum |d| = 8; c = (-3, 0, 0, 3) (the two 3s: one below, one above, the tie counts 0); sum c d = 9 + 9 = 18
#   crps = 8 / 4 - 18 / 16 = 0.875; rank = 3, ties = 0
#   d crps / d x = sign(d) / 4 - c / 16 = (-1/4 + 3/16, -1/4, -1/4, 1/4 - 3/16) = (-1/16, -1/4, -1/4, 1/16)
#   d crps / d y = -(-1 - 1 - 1 + 1) / 4 = 1/2
# case 2, a sample equal to the observation: x = (6, 2, 4, 0), y = 4
#   d = (2, -2, 0, -4), sum |d| = 8; c = (3, -1, 1, -3); sum c d = 6 + 2 + 0 + 12 = 20
#   crps = 8 / 4 - 20 / 16 = 0.75; rank = 2, ties = 1
#   d crps / d x = (1/4 - 3/16, -1/4 + 1/16, 0 - 1/16, -1/4 + 3/16) = (1/16, -3/16, -1/16, -1/16)
#   d crps / d y = -(1 - 1 + 0 - 1) / 4 = 1/4
EXACT = [((1., 3., 3., 7.), 4., 0.875, 3., 0., (-1 / 16, -1 / 4, -1 / 4, 1 / 16), 1 / 2),
         ((6., 2., 4., 0.), 4., 0.75, 2., 1., (1 / 16, -3 / 16, -1 / 16, -1 / 16), 1 / 4)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_exact_known_answers_with_a_duplicate_and_with_a_tie_against_the_target(dtype):
    x = torch.tensor([c[0] for c in EXACT], dtype=dtype).reshape(8, 1).requires_grad_(True)       # (G S, W) = (2 * 4, 1)
    y = torch.tensor([[c[1]] for c in EXACT], dtype=dtype, requires_grad=True)
    crps, rank, ties = S.sample_crps(x, 4, y, fair=False, rank=True)
    assert crps.dtype == dtype and rank.dtype == ties.dtype == torch.float32
    assert not rank.requires_grad and not ties.requires_grad
    assert crps.detach().reshape(-1).tolist() == [c[2] for c in EXACT]
    assert rank.reshape(-1).tolist() == [c[3] for c in EXACT] and ties.reshape(-1).tolist() == [c[4] for c in EXACT]
    crps.sum().backward()
    assert x.grad.reshape(2, 4).tolist() == [list(c[5]) for c in EXACT]
    assert y.grad.reshape(-1).tolist() == [c[6] for c in EXACT]
    # the fair estimator of case 1: D = 3, crps = 2 - 18 / 12 = 0.5
    assert S.sample_crps(x.detach()[:4], 4, y.detach()[:1]).item() == 0.5
    # quantiles of case 1 at q = 0, 1/2, 1: positions 0, 1.5 (between the two 3s), 3
    q = S.sample_quantiles(x.detach()[:4], 4, [0.0, 0.5, 1.0])
    assert q.shape == (3, 1, 1) and q.reshape(-1).tolist() == [1.0, 3.0, 7.0]
    xq = x.detach()[:4].clone().requires_grad_(True)
    S.sample_quantiles(xq, 4, [0.5])[0].sum().backward()      # pos = 1.5: ranks 1 and 2 are the two 3s, lower index first
    assert xq.grad.reshape(-1).tolist() == [0.0, 0.5, 0.5, 0.0]


def _pairwise64(x, y, fair):
    """Brute-force float64 statement: mean |x - y| - sum_ij |x_i - x_j| / (2 N D); x (G, N, W), y (G, W)."""
    N = x.shape[1]
    D = N - 1 if fair else N
    return (x - y[:, None]).abs().sum(1) / N - (x[:, :, None] - x[:, None, :]).abs().sum((1, 2)) / (2 * N * D)


@pytest.mark.parametrize('fair', [True, False])
def test_random_inputs_against_the_pairwise_statement_in_float64(fair):
    G, Sn, W = 5, 7, 3
    gen = torch.Generator().manual_seed(11)
    x32 = torch.randn(G * Sn, W, generator=gen)
    y32 = torch.randn(G, W, generator=gen)
    x64, y64 = x32.double().requires_grad_(True), y32.double().requires_grad_(True)
    ref = _pairwise64(x64.reshape(G, Sn, W), y64, fair)
    gx_ref, gy_ref = torch.autograd.grad(ref.sum(), (x64, y64))
    for dtype, tol in ((torch.float64, 1e-14), (torch.float32, (2 * Sn + 4) * U * 8)):      # (standard normal x, y: A + B' < 8)
        x, y = x32.to(dtype).requires_grad_(True), y32.to(dtype).requires_grad_(True)
        crps, rank, ties = S.sample_crps(x, Sn, y, fair=fair, rank=True)
        assert crps.shape == (G, W) and crps.dtype == dtype
        assert float((crps.detach().double() - ref.detach()).abs().max()) <= tol
        assert torch.equal(rank, (x32.reshape(G, Sn, W) < y32[:, None]).sum(1).float()) and float(ties.sum()) == 0
        gx, gy = torch.autograd.grad(crps.sum(), (x, y))
        assert float((gx.double() - gx_ref).abs().max()) <= tol and float((gy.double() - gy_ref).abs().max()) <= tol
    # leading axes fold into the groups
    stacked = S.sample_crps(torch.stack([x32, 2 * x32]), Sn, torch.stack([y32, 2 * y32]), fair=fair)
    assert stacked.shape == (2, G, W) and torch.equal(stacked[0], S.sample_crps(x32, Sn, y32, fair=fair))


def test_quantiles_against_torch_quantile_in_float64():
    G, Sn, W = 5, 7, 3
    gen = torch.Generator().manual_seed(12)
    x32 = torch.randn(G * Sn, W, generator=gen)
    qs = (0, 0.1, 0.5, 0.9, 1)
    ref = torch.quantile(x32.double().reshape(G, Sn, W), torch.tensor(qs, dtype=torch.float64), dim=1, interpolation='linear')
    amax = float(x32.abs().max())
    for dtype in (torch.float64, torch.float32):      # (frac is a float32 in both: 3 u (|x_(k)| + |x_(k+1)|) covers it)
        got = S.sample_quantiles(x32.to(dtype), Sn, qs)
        assert got.shape == (5, G, W) and got.dtype == dtype
        assert float((got.double() - ref).abs().max()) <= 3 * U * 2 * amax
        assert torch.equal(got[0], x32.to(dtype).reshape(G, Sn, W).min(1).values)
        assert torch.equal(got[-1], x32.to(dtype).reshape(G, Sn, W).max(1).values)
    x = x32.double().requires_grad_(True)
    S.sample_quantiles(x, Sn, [0.1])[0].sum().backward()      # pos = 0.6: 0.4 to rank 0, 0.6 to rank 1, zeros elsewhere
    g = x.grad.reshape(G, Sn, W)
    assert int((g != 0).sum()) == 2 * G * W
    assert float((g.sum(1) - 1).abs().max()) < 1e-7
    assert engine.quantile_positions([0, 0.1, 1], 7) == ([0, 0, 6], [0.0, float(np.float32(0.6000000000000001)), 0.0])
    for bad in ([], [1.5], [-0.1], [float('nan')]):
        with pytest.raises(ValueError, match='q must'):
            S.sample_quantiles(x32, Sn, bad)
    assert S.sample_quantiles(x32, Sn, [i / 9 for i in range(10)]).shape == (10, G, W)      # more than 8 levels: tensor ops


def test_pooled_members_equal_the_permuted_single_member_call():
    O, M, G, Sn, W = 2, 3, 2, 4, 5
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(O, M, G * Sn, W, generator=gen)
    x[0, 1, 2] = x[0, 0, 1]      # (a tie across members)
    y = torch.randn(O, G, W, generator=gen)
    flat = x.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W).contiguous()
    for fair in (True, False):
        a = S.sample_crps(x, Sn, y, fair=fair, members=M, rank=True)
        b = S.sample_crps(flat, M * Sn, y, fair=fair, rank=True)
        assert a[0].shape == (O, G, W) and all(torch.equal(u, v) for u, v in zip(a, b))
    qa, qb = S.sample_quantiles(x, Sn, [0.25, 0.5], members=M), S.sample_quantiles(flat, M * Sn, [0.25, 0.5])
    assert qa.shape == (2, O, G, W) and torch.equal(qa, qb)
    xa, xb = x.clone().requires_grad_(True), flat.clone().requires_grad_(True)
    S.sample_crps(xa, Sn, y, members=M).sum().backward()
    S.sample_crps(xb, M * Sn, y).sum().backward()
    assert torch.equal(xa.grad.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), xb.grad)


def test_shape_errors_are_value_errors():
    x, y = torch.zeros(12, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match='whole number'):
        S.sample_crps(x, 5, y)
    with pytest.raises(ValueError, match='target'):
        S.sample_crps(x, 3, torch.zeros(3, 3))
    with pytest.raises(ValueError, match='at least 2'):
        S.sample_crps(x, 1, torch.zeros(12, 3))
    assert S.sample_crps(x, 1, torch.zeros(12, 3), fair=False).shape == (12, 3)
    with pytest.raises(ValueError, match='members'):
        S.sample_crps(x, 3, y, members=0)
    with pytest.raises(ValueError, match='members'):
        S.sample_crps(torch.zeros(2, 12, 3), 3, y, members=3)
    with pytest.raises(ValueError, match='samples'):
        S.sample_quantiles(x, 0, [0.5])
    assert S.sample_crps(torch.zeros(0, 3), 2, torch.zeros(0, 3)).shape == (0, 3)
    assert S.sample_quantiles(torch.zeros(0, 3), 2, [0.5]).shape == (1, 0, 3)


def test_crps_loss_on_forecasting_shaped_predictions():
    B, Sn, T_out, Cn = 3, 4, 5, 2
    gen = torch.Generator().manual_seed(14)
    pred = torch.randn(B * Sn, T_out, Cn, generator=gen, requires_grad=True)
    true = torch.randn(B, T_out, Cn, generator=gen)
    loss = S.crps_loss(Sn)(pred, true)
    assert loss.shape == () and torch.equal(loss, S.sample_crps(pred.reshape(B * Sn, T_out * Cn), Sn, true.reshape(B, T_out * Cn)).mean())
    loss.backward()
    assert pred.grad.shape == pred.shape and float(pred.grad.abs().sum()) > 0
    assert torch.equal(S.crps_loss(Sn, fair=False)(pred, true),
                       S.sample_crps(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), fair=False).mean())
    with pytest.raises(ValueError, match='crps_loss'):
        S.crps_loss(Sn)(pred[:-1], true)
    with pytest.raises(ValueError, match='crps_loss'):
        S.crps_loss(Sn)(pred, true[:-1])
    # an Ensemble's (M, B S, ...) output: the members' paths are pooled
    M = 2
    pm = torch.randn(M, B * Sn, T_out, Cn, generator=gen)
    assert torch.equal(S.crps_loss(Sn, members=M)(pm, true),
                       S.sample_crps(pm.reshape(M, B * Sn, -1), Sn, true.reshape(B, -1), members=M).mean())
    with pytest.raises(ValueError, match='crps_loss'):
        S.crps_loss(Sn, members=3)(pm, true)
    with pytest.raises(ValueError, match='samples'):
        S.crps_loss(0)
