"""The masked Gaussian likelihood of sample paths on the host: the entry points snsde_sample_loglik / _backward (declared, exported,
bound, validating before they launch), and sample_loglik / iwae_loss on CPU tensors - the tensor-op statement of the definition -
against the interpolation benchmark's own objective (tests/golden/loglik.npz), the select semantics, and gradcheck.  No GPU compute.

The fixture bound.  loglik.npz holds what the reference computes in float32 (u = 2^-24); our side runs in float64 and is exact at
that scale, so the whole difference is the reference's rounding.  One element's term -1/2 (log 2 pi + logvar + (x - mean)^2 /
exp(logvar)) mask: logvar = 2 logf(0.1f) is off 2 log(0.1) by at most 2 (u + u |log 0.1|) < 7 u absolutely, so exp(logvar) by
8 u relatively; the quotient collects the difference (u), its square (2 u), exp (8 u) and the division (u); log 2 pi one
rounding; two additions, the product with -1/2 (exact) and with the mask (exact for 0 / 1): every term is within 24 u of
(log 2 pi + |logvar| + d^2 / var) / 2.  The T D = 15 terms of a row are summed by torch in float32: at most 15 u more on the sum
of the absolute terms.  Hence |logpx_ref - logpx| <= (24 + T D) u A, A = sum_v mask_v (log 2 pi + |logvar| + d_v^2 / var) / 2,
and one u |logpx| more for the division under norm.  The loss: a = logpx - kl_coef kl adds u (|logpx| + 2 |kl_coef kl|) per
entry, logsumexp is 1-Lipschitz in the largest entry error and rounds its own max / exp / sum / log within 8 u (max |a| + 2),
the mean over rows and the subtraction of log k within 8 u (max |a| + 2) more.  The MSE: mean over k, difference, square,
product, a sum of B T D = 60 non-negative terms and one division: within (2 k + 66) u of itself."""
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
NAMES = ('snsde_sample_loglik', 'snsde_sample_loglik_backward')
U = 2.0 ** -24
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loglik.npz'))


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (17, 20)):
        assert f'SNSDE_API int {name}(' in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f' T {name}\n' in dyn
        assert len(getattr(lib, name).argtypes) == arity
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)
    assert S.sample_loglik is engine.sample_loglik and S.iwae_loss is train.iwae_loss


def _fwd(lib, outer=1, members=1, groups=1, samples=4, width=1, logvar=-4.6, inv_var=100.0, ys=4096, target=4096, mask=4096, logpx=4096,
         count=4096, bound=4096, sqerr=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_loglik(p(ys), p(target), p(mask), None, outer, members, groups, samples, width, logvar, inv_var, 0, p(logpx),
                                   p(count), p(bound), p(sqerr), None)


def _bwd(lib, outer=1, members=1, groups=1, samples=4, width=1, logvar=-4.6, inv_var=100.0, ys=4096, target=4096, mask=4096, logpx=4096,
         count=4096, gys=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_loglik_backward(None, None, p(ys), p(target), p(mask), None, p(logpx), p(count), outer, members, groups,
                                            samples, width, logvar, inv_var, 1, p(gys), None, None, None)


def test_the_entry_points_validate_before_they_launch():
    lib = _lib.lib()
    inf, nan = float('inf'), float('nan')
    for fn in (_fwd, _bwd):
        for name in ('ys', 'target', 'mask', 'logpx', 'count'):
            assert fn(lib, **{name: 0}) == ERR_NULL, name
        assert fn(lib, outer=0) == ERR_DIMS and fn(lib, members=0) == ERR_DIMS
        assert fn(lib, groups=0) == ERR_DIMS and fn(lib, samples=0) == ERR_DIMS
        assert fn(lib, width=0) == ERR_DIMS and fn(lib, groups=-3) == ERR_DIMS
        assert fn(lib, samples=257) == ERR_DIMS                                # N > 256
        assert fn(lib, samples=1, members=257) == ERR_DIMS
        assert fn(lib, samples=129, members=2) == ERR_DIMS                     # N = 258
        assert fn(lib, groups=2 ** 62, width=8) == ERR_DIMS                    # 63-bit overflow
        assert fn(lib, outer=2 ** 40, groups=2 ** 20, width=64) == ERR_DIMS
        assert fn(lib, inv_var=0.0) == ERR_DIMS and fn(lib, inv_var=-1.0) == ERR_DIMS      # std = inf, a negative variance
        assert fn(lib, inv_var=inf, logvar=-inf) == ERR_DIMS                              # std = 0
        assert fn(lib, logvar=nan) == ERR_DIMS and fn(lib, inv_var=nan) == ERR_DIMS
    assert _fwd(lib, bound=0) == ERR_NULL and _fwd(lib, sqerr=0) == ERR_NULL
    assert _bwd(lib, gys=0) == ERR_NULL


# ---- the reference's objective ----------------------------------------------------------------------------------------------------------

def _gold_case(k):
    """The fixture's (k, B, T, D) prediction as path-minor rows b S + s, float64; the NaN-marked target; A of the bound."""
    data, mask, pred = (torch.from_numpy(GOLD[f'k{k}/{n}']).double() for n in ('data', 'mask', 'pred'))
    B, T, D = data.shape
    rows = pred.permute(1, 0, 2, 3).reshape(B * k, T, D)                        # (B k, T, D): row b k + s
    marked = torch.where(mask != 0, data, torch.full_like(data, float('nan')))
    logvar = 2.0 * math.log(float(GOLD['std']))
    d2 = (data.unsqueeze(0) - pred).square() * math.exp(-logvar)
    A = (0.5 * mask * (math.log(2 * math.pi) + abs(logvar) + d2)).sum((-2, -1))      # (k, B)
    return data, mask, rows, marked, A, (B, T, D)


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('k', [1, 3])
def test_the_tensor_op_statement_against_the_reference_objective(k, norm):
    """logpx, the loss at kl_coef 0 and 0.5, and the MSE of the sample mean, within the bound the module docstring derives."""
    data, mask, rows, marked, A, (B, T, D) = _gold_case(k)
    std = float(GOLD['std'])
    key = f'k{k}/norm{int(norm)}'
    ref_logpx, kl = GOLD[f'{key}/logpx'].astype(np.float64), GOLD[f'{key}/analytic_kl'].astype(np.float64)      # (k, B), (B,)
    ys, tg, mk = rows.reshape(B * k, T * D), data.reshape(B, T * D), mask.reshape(B, T * D)
    bound, logpx, count, sqerr = engine.sample_loglik_tensor_ops(ys, k, tg, mk, std=std, norm=norm, stats=True)
    assert logpx.shape == (B, k) and bound.shape == count.shape == sqerr.shape == (B,) and logpx.dtype == torch.float64
    cnt = mask.sum((-2, -1))
    assert torch.equal(count, cnt)
    E = (24 + T * D) * U * A.numpy() / (cnt.numpy() if norm else 1.0) + (U * np.abs(ref_logpx) if norm else 0.0)      # (k, B)
    err = np.abs(logpx.numpy().T - ref_logpx)
    print(f'loglik fixture k={k} norm={norm}: logpx err / bound max {np.max(err / E):.3f}')
    assert (err <= E).all()
    # the time-major layout of a solve, the NaN-marked target and mask=None: the same numbers
    b2, l2, c2, s2 = S.sample_loglik(rows.permute(1, 0, 2).contiguous(), k, marked.permute(1, 0, 2).contiguous(), std=std, norm=norm, stats=True)
    assert float((l2 - logpx).abs().max()) <= 1e-12 * float(logpx.abs().max()) and torch.equal(c2, count)
    assert float((b2 - bound).abs().max()) <= 1e-12 * float(bound.abs().max()) and float((s2 - sqerr).abs().max()) <= 1e-13
    for kl_coef in (0.0, 0.5):
        want = float(GOLD[f'{key}/loss_kl{kl_coef}'])
        lw = None if kl_coef == 0.0 else (-kl_coef * torch.from_numpy(kl)).unsqueeze(1).expand(B, k).contiguous()
        loss = -float(engine.sample_loglik_tensor_ops(ys, k, tg, mk, std=std, log_weight=lw, norm=norm).mean())
        amax = float(np.abs(ref_logpx - kl_coef * kl).max())
        El = float((E + U * (np.abs(ref_logpx) + 2 * kl_coef * np.abs(kl))).max()) + 16 * U * (amax + 2)
        print(f'loglik fixture k={k} norm={norm} kl_coef={kl_coef}: loss {loss:.6f} reference {want:.6f} err / bound {abs(loss - want) / El:.3f}')
        assert abs(loss - want) <= El
        if kl_coef == 0.0:
            got = float(S.iwae_loss(k, std=std, norm=norm)(rows, marked))
            assert abs(got - want) <= El and abs(got - loss) <= 1e-12 * abs(loss)
            assert float(S.iwae_loss(k, std=std, norm=norm)(rows, (data, mask))) == pytest.approx(got, rel=1e-12)
    mse, want = float(sqerr.sum() / count.sum()), float(GOLD[f'k{k}/mse'])
    assert abs(mse - want) <= (2 * k + 66) * U * want


# ---- the definition itself ---------------------------------------------------------------------------------------------------------------

def _random_case(seed, O, G, Sn, W, M=1, dtype=torch.float64, frac=False):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*((O,) if O else ()), *((M,) if M > 1 else ()), G * Sn, W, generator=gen, dtype=dtype)
    y = torch.randn(*((O,) if O else ()), G, W, generator=gen, dtype=dtype)
    m = (torch.rand(y.shape, generator=gen) > 0.4).to(dtype)
    if frac:
        m = m * (0.25 + torch.rand(y.shape, generator=gen, dtype=dtype))
    lw = 0.5 * torch.randn(G, M * Sn, generator=gen, dtype=dtype)
    return x, y, m, lw


@pytest.mark.parametrize('norm', [False, True])
def test_unobserved_elements_are_selected_out_bit_for_bit_and_get_exact_zero_gradients(norm):
    O, G, Sn, W = 2, 3, 4, 5
    x, y, m, lw = _random_case(31, O, G, Sn, W, dtype=torch.float32)
    hide_x = (m == 0).repeat_interleave(Sn, dim=1)                      # (O, G Sn, W): unobserved positions of every path
    poison = torch.tensor([float('nan'), float('inf'), -float('inf')])
    outs, grads = [], []
    for planted in (False, True):
        xx, yy = x.clone(), y.clone()
        if planted:
            xx[hide_x] = poison[torch.arange(int(hide_x.sum())) % 3]
            yy[m == 0] = poison[torch.arange(int((m == 0).sum())) % 3]
        else:
            xx[hide_x] = 0.0
            yy[m == 0] = 0.0
        xx.requires_grad_(True), yy.requires_grad_(True)
        lwg = lw.float().clone().requires_grad_(True)
        out = S.sample_loglik(xx, Sn, yy, m, std=0.3, log_weight=lwg, norm=norm, stats=True)
        g = torch.autograd.grad(out[0].sum() + (out[1] * out[1].detach().cos()).sum(), (xx, yy, lwg))
        outs.append(out), grads.append(g)
    for a, b in zip(outs[0], outs[1]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    for a, b in zip(grads[0], grads[1]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    assert float(grads[1][0][hide_x].abs().max()) == 0 and float(grads[1][1][m == 0].abs().max()) == 0
    assert float(grads[1][0][~hide_x].abs().min()) > 0
    # mask=None is ~isnan(target)
    marked = torch.where(m != 0, y, torch.full_like(y, float('nan')))
    a = S.sample_loglik(x, Sn, marked, std=0.3, norm=norm, stats=True)
    b = S.sample_loglik(x, Sn, marked, (~torch.isnan(marked)).float(), std=0.3, norm=norm, stats=True)
    c = S.sample_loglik(x, Sn, y, m, std=0.3, norm=norm, stats=True)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w) and bool(torch.isfinite(u).all())
    assert torch.equal(S.sample_loglik(x, Sn, y, m != 0, std=0.3, norm=norm), c[0])      # a bool mask


@pytest.mark.parametrize('norm', [False, True])
def test_a_group_with_nothing_observed(norm):
    G, Sn, W = 3, 4, 5
    x, y, m, lw = _random_case(32, 0, G, Sn, W)
    m[1] = 0.0
    y[1] = float('nan')
    x.requires_grad_(True), y.requires_grad_(True), lw.requires_grad_(True)
    bound, logpx, count, sqerr = S.sample_loglik(x, Sn, y, m, log_weight=lw, norm=norm, stats=True)
    assert float(logpx.detach()[1].abs().max()) == 0 and float(count[1]) == 0 and float(sqerr[1]) == 0
    assert float(bound.detach()[1]) == pytest.approx(float(torch.logsumexp(lw.detach()[1], 0)) - math.log(Sn), rel=1e-14)
    assert bool(torch.isfinite(bound).all()) and bool(torch.isfinite(logpx).all())
    gx, gy = torch.autograd.grad(bound.sum() + logpx.sum(), (x, y))
    assert float(gx[Sn:2 * Sn].abs().max()) == 0 and float(gy[1].abs().max()) == 0
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all()) and float(gx[:Sn].abs().max()) > 0
    # without weights the bound of an empty group is log N - log N
    assert float(S.sample_loglik(x.detach(), Sn, y.detach(), m, norm=norm)[1]) == pytest.approx(0.0, abs=1e-15)


def test_a_nan_in_an_observed_element_poisons_its_own_group_only():
    G, Sn, W = 3, 4, 5
    x, y, m, lw = _random_case(33, 0, G, Sn, W)
    m[:] = 1.0
    x[Sn + 2, 3] = float('nan')
    x[2 * Sn + 1, 0] = float('inf')
    bound, logpx, count, sqerr = S.sample_loglik(x, Sn, y, m, stats=True)
    assert bool(torch.isnan(logpx[1, 2])) and bool(torch.isnan(bound[1])) and bool(torch.isnan(sqerr[1]))
    assert bool(torch.isfinite(logpx[1, [0, 1, 3]]).all()) and bool(torch.isfinite(logpx[0]).all())
    assert float(logpx[2, 1]) == -float('inf') and bool(torch.isfinite(bound[[0, 2]]).all()) and bool(torch.isfinite(sqerr[0]))
    xs = x.clone()
    xs[2 * Sn:] = float('inf')      # every path of the group: logsumexp of all -Inf
    assert float(S.sample_loglik(xs, Sn, y, m)[2]) == -float('inf')


def test_pooled_members_equal_the_hand_pooled_tensor():
    O, M, G, Sn, W = 2, 2, 3, 4, 5
    x, y, m, lw = _random_case(34, O, G, Sn, W, M=M, frac=True)
    flat = x.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W).contiguous()
    for norm in (False, True):
        a = S.sample_loglik(x, Sn, y, m, members=M, log_weight=lw, norm=norm, stats=True)
        b = S.sample_loglik(flat, M * Sn, y, m, log_weight=lw, norm=norm, stats=True)
        assert a[1].shape == (G, M * Sn)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    xa, xb = x.clone().requires_grad_(True), flat.clone().requires_grad_(True)
    S.sample_loglik(xa, Sn, y, m, members=M, log_weight=lw).sum().backward()
    S.sample_loglik(xb, M * Sn, y, m, log_weight=lw).sum().backward()
    assert torch.equal(xa.grad.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), xb.grad)
    assert float(xa.grad.abs().max()) > 0


@pytest.mark.parametrize('norm', [False, True])
def test_gradcheck_of_the_tensor_op_statement_with_fractional_weights(norm):
    O, G, Sn, W = 2, 2, 3, 3
    x, y, m, lw = _random_case(35, O, G, Sn, W, frac=True)
    m[0, 0, 1] = 0.0
    y[0, 0, 1] = float('nan')      # an unobserved, NaN-marked element stays out of the check's perturbations' way: its gradient is 0
    x.requires_grad_(True), lw.requires_grad_(True)
    yz = torch.where(m != 0, y, torch.zeros_like(y)).requires_grad_(True)

    def both(xx, yy, ww):
        bound, logpx, count, sqerr = engine.sample_loglik_tensor_ops(xx, Sn, yy, m, std=0.7, log_weight=ww, norm=norm, stats=True)
        return bound, logpx
    assert torch.autograd.gradcheck(both, (x, yz, lw), eps=1e-6, atol=1e-6, rtol=1e-6)
    # the formulas of the adjoint, written out
    bound, logpx, count, sqerr = engine.sample_loglik_tensor_ops(x, Sn, yz, m, std=0.7, log_weight=lw, norm=norm, stats=True)
    gb, gl = torch.randn(G, dtype=torch.float64), torch.randn(G, Sn, dtype=torch.float64)
    gx, gy, gw = torch.autograd.grad((bound * gb).sum() + (logpx * gl).sum(), (x, yz, lw))
    p = torch.softmax(logpx + lw, dim=-1).detach()
    c = (gl + gb[:, None] * p) / (count[:, None] if norm else 1.0)                                  # (G, N)
    d = yz.detach()[:, :, None, :] - x.detach().reshape(O, G, Sn, W)                                 # (O, G, N, W)
    want = c[None, :, :, None] * m[:, :, None, :] * d / 0.49
    assert float((gx.reshape(O, G, Sn, W) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((gy + want.sum(2)).abs().max()) <= 1e-12 * float(want.abs().max()) * Sn
    assert float((gw - gb[:, None] * p).abs().max()) <= 1e-14


def test_argument_errors_are_value_errors():
    x, y = torch.zeros(12, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match='whole number'):
        S.sample_loglik(x, 5, y)
    with pytest.raises(ValueError, match='target'):
        S.sample_loglik(x, 3, torch.zeros(4))
    with pytest.raises(ValueError, match='mask'):
        S.sample_loglik(x, 3, y, torch.ones(4, 2))
    for std in (0.0, -1.0, float('inf'), float('nan'), True, '0.1', None):
        with pytest.raises(ValueError, match='std'):
            S.sample_loglik(x, 3, y, std=std)
    with pytest.raises(ValueError, match='log_weight'):
        S.sample_loglik(x, 3, y, log_weight=torch.zeros(4))
    with pytest.raises(ValueError, match='log_weight'):
        S.sample_loglik(x, 3, y, log_weight=torch.zeros(3, 4))
    with pytest.raises(ValueError, match='members'):
        S.sample_loglik(x, 3, y, members=0)
    with pytest.raises(ValueError, match='samples'):
        S.sample_loglik(x, 0, y)
    out = S.sample_loglik(x, 3, y, log_weight=torch.zeros(4, 3), stats=True)
    assert out[0].shape == (4,) and out[1].shape == (4, 3) and out[2].shape == (4,) and out[3].shape == (4,)
    assert S.sample_loglik(torch.zeros(2, 12, 3), 3, torch.zeros(2, 4, 3)).shape == (4,)      # leading axes join the vector


def test_iwae_loss_shapes_masks_and_errors():
    B, Sn, T_out, Cn = 3, 4, 5, 2
    gen = torch.Generator().manual_seed(36)
    pred = torch.randn(B * Sn, T_out, Cn, generator=gen, requires_grad=True)
    true = torch.randn(B, T_out, Cn, generator=gen)
    true[0, 1, 0] = true[2, :, 1] = float('nan')
    loss = S.iwae_loss(Sn, std=0.5)(pred, true)
    want = -S.sample_loglik(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), std=0.5).mean()
    assert loss.shape == () and bool(torch.isfinite(loss)) and torch.equal(loss, want)
    loss.backward()
    hidden = torch.isnan(true).repeat_interleave(Sn, 0)
    assert pred.grad.shape == pred.shape and float(pred.grad[hidden].abs().max()) == 0 and float(pred.grad[~hidden].abs().min()) > 0
    values, mask = torch.nan_to_num(true, 0.0), (~torch.isnan(true)).float()
    assert torch.equal(S.iwae_loss(Sn, std=0.5)(pred, (values, mask)), loss)
    assert torch.equal(S.iwae_loss(Sn, std=0.5, norm=True)(pred, true),
                       -S.sample_loglik(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), std=0.5, norm=True).mean())
    with pytest.raises(ValueError, match='iwae_loss'):
        S.iwae_loss(Sn)(pred[:-1], true)
    with pytest.raises(ValueError, match='iwae_loss'):
        S.iwae_loss(Sn)(pred, (values, mask[:-1]))
    M = 2
    pm = torch.randn(M, B * Sn, T_out, Cn, generator=gen)      # an Ensemble's (M, B S, ...) output: the members' paths are pooled
    assert torch.equal(S.iwae_loss(Sn, members=M)(pm, true),
                       -S.sample_loglik(pm.reshape(M, B * Sn, -1), Sn, true.reshape(B, -1), members=M).mean())
    with pytest.raises(ValueError, match='samples'):
        S.iwae_loss(0)
