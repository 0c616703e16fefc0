"""snsde_ensemble_stats / snsde_ensemble_stats_backward on the GPU: ys viewed as (outer, M, groups, S, width) reduced to the
predictive mean, the within-member (aleatoric) and the between-member (epistemic) variance, each (outer, groups, width).

Shapes: (2, 3, 5, 4, 64) - the four-columns-per-lane kernel, outer > 1 and a group count that is no power of two; (1, 2, 3, 2, 7) - a width that is no multiple of four: one column per lane; (1, 4, 1, 3, 1) - one
group of one column; and a view that is not 16-byte aligned at width 64.  u = 2^-24 throughout."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.score_special_cases import ENSEMBLE_STATS_SHAPES

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

SHAPES = ENSEMBLE_STATS_SHAPES
U = 2.0 ** -24


def _data(shape):
    O, M, G, Sn, W = shape
    rng = np.random.default_rng(O + M + G + Sn + W)
    # members whose means lie apart (0.7 m) around paths of spread 3: neither variance part is negligible against the other
    x = (3.0 * rng.standard_normal(shape) + 1.0 + 0.7 * np.arange(M).reshape(1, M, 1, 1, 1)).astype(np.float32)
    return x, torch.from_numpy(x).to(DEV).reshape(O, M, G * Sn, W)


def _fp64_parts(x):
    """From the float64 values of the float32 inputs: member means and their error bound e_m (the mean bound of
    tests/test_gpu_samples.py::test_sample_stats_against_float64), the mean of means and the bound D_m on the error of a computed
    deviation mean_m^ - mean^."""
    O, M, G, Sn, W = x.shape
    x64 = x.astype(np.float64)
    mm = x64.mean(3)                                                # (O, M, G, W)
    e_m = (Sn + 1) * U * np.abs(x64).sum(3) / Sn                    # |mean_m^ - mean_m| <= e_m
    mu = mm.mean(1)                                                 # (O, G, W)
    # mean^ sums the M computed member means in order and divides once: as the bound above with S -> M, on terms |mean_m^| <=
    # |mean_m| + e_m, plus the inherited errors e_m averaged
    e_mu = (M + 1) * U * (np.abs(mm) + e_m).sum(1) / M + e_m.sum(1) / M
    return x64, mm, e_m, mu, e_mu


@pytest.mark.parametrize('shape', SHAPES)
def test_mean_and_within_are_sample_stats_per_member_then_an_ascending_float32_loop(shape):
    O, M, G, Sn, W = shape
    x, xd = _data(shape)
    mean, within, between = S.ensemble_stats(xd, M, Sn)
    again = S.ensemble_stats(xd, M, Sn)
    torch.cuda.synchronize()
    assert tuple(mean.shape) == tuple(within.shape) == tuple(between.shape) == (O, G, W)
    assert all(torch.equal(a, b) for a, b in zip((mean, within, between), again))      # two launches: identical bits
    # (the loop runs in numpy float32 on the host: IEEE additions and one correctly rounded division, which a tensor division by a
    #  Python scalar - a multiplication by the reciprocal - is not)
    msum, wsum = np.zeros((O, G, W), np.float32), np.zeros((O, G, W), np.float32)
    for m in range(M):      # m ascending, float32 adds
        sm, sv = S.sample_stats(xd[:, m].contiguous(), Sn)
        msum = msum + sm.cpu().numpy()
        wsum = wsum + sv.cpu().numpy()
    assert msum.dtype == np.float32 and wsum.dtype == np.float32
    assert np.array_equal(mean.cpu().numpy(), msum / np.float32(M))
    assert np.array_equal(within.cpu().numpy(), wsum / np.float32(M))
    # NULL outputs: each subset gives the same bits for what it returns
    m1, w1, b1 = S.ensemble_stats(xd, M, Sn, within=False)
    m2, w2, b2 = S.ensemble_stats(xd, M, Sn, between=False)
    m3, w3, b3 = S.ensemble_stats(xd, M, Sn, within=False, between=False)
    assert w1 is None and b2 is None and w3 is None and b3 is None
    assert torch.equal(m1, mean) and torch.equal(m2, mean) and torch.equal(m3, mean) and torch.equal(b1, between) and torch.equal(w2, within)
    out = torch.full((O, G, W), 7.0, device=DEV)      # ... and the C entry point with mean = NULL writes the one output it was given
    rc = engine._lib.lib().snsde_ensemble_stats(xd.data_ptr(), O, M, G, Sn, W, None, None, out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, between)


@pytest.mark.parametrize('shape', SHAPES)
def test_between_against_float64(shape):
    """between^ = fl(sum_m fma(d_m^, d_m^, .) / (M - 1)) with d_m^ = fl(mean_m^ - mean^).  With a_m = mean_m - mean (exact) and
    |d_m^ - a_m| <= D_m = e_m + e_mu + u (|a_m| + e_m + e_mu) (the two inherited errors and the subtraction's rounding), the sum of
    squares T^ = sum (a_m + delta_m)^2 differs from T = sum a_m^2 by at most R = sum (2 |a_m| D_m + D_m^2); the M fused
    multiply-adds of non-negative terms and the division add a relative (M + 1) u, taken as gamma = (M + 4) u as in
    test_sample_stats_against_float64.  Hence |between^ - between| <= (gamma (T + R) + R) / (M - 1)."""
    O, M, G, Sn, W = shape
    x, xd = _data(shape)
    _, _, between = S.ensemble_stats(xd, M, Sn, within=False)
    x64, mm, e_m, mu, e_mu = _fp64_parts(x)
    a = mm - mu[:, None]
    D = e_m + e_mu[:, None]
    D = D + U * (np.abs(a) + D)
    T, R = (a ** 2).sum(1), (2 * np.abs(a) * D + D ** 2).sum(1)
    bound = ((M + 4) * U * (T + R) + R) / (M - 1)
    err = np.abs(between.cpu().numpy().astype(np.float64) - T / (M - 1))
    print(f'ensemble_stats {shape}: between err / bound max {np.max(err / bound):.3f}')
    assert (err <= bound).all()
    assert (T > 0).all()


def test_an_unaligned_view_takes_the_scalar_kernel_and_gives_the_same_numbers():
    O, M, G, Sn, W = 1, 3, 2, 3, 64
    buf = torch.randn(M * G * Sn * W + 1, device=DEV)
    a = S.ensemble_stats(buf[1:].reshape(M, G * Sn, W), M, Sn)                 # 4 bytes off a 16-byte boundary
    b = S.ensemble_stats(buf[1:].clone().reshape(M, G * Sn, W), M, Sn)         # aligned copy: four columns per lane
    assert buf[1:].data_ptr() % 16 != 0
    assert all(tuple(t.shape) == (G, W) for t in a) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize('shape', SHAPES)
def test_backward_against_float64_autograd(shape):
    """grad_ys = A + Cw (x - mean_m^) + Cb (mean_m^ - mean^), A = g_mean / (M S), Cw = 2 g_within / ((S - 1) M),
    Cb = 2 g_between / ((M - 1) S), against float64 autograd of the forward's formulas on the same float32 inputs.  Each
    coefficient takes at most three roundings (a product by two is exact), each difference one, and the two fused multiply-adds
    round once each over everything they hold: a relative 6 u on every term to first order, 8 u with the second-order terms; the
    inherited errors of the computed means enter through the differences, |x - mean_m^| within e_m and |mean_m^ - mean^| within
    e_m + e_mu.  Hence |err| <= 8 u (|A| + |Cw| |x - mean_m| + |Cb| |a_m|) + (1 + 8 u) (|Cw| e_m + |Cb| (e_m + e_mu)), plus 1e-12
    times the same magnitudes for the float64 reference's own rounding (its terms through the means of the deviations, zero in
    exact arithmetic)."""
    O, M, G, Sn, W = shape
    x, xd = _data(shape)
    gen = torch.Generator().manual_seed(9)
    gm, gw, gb = (torch.randn(O, G, W, generator=gen) for _ in range(3))
    xa = xd.clone().requires_grad_(True)
    mean, within, between = S.ensemble_stats(xa, M, Sn)
    assert type(mean.grad_fn).__name__ == '_EnsembleStatsBackward'
    (mean * gm.to(DEV)).sum().backward(retain_graph=True)
    g_mean_only = xa.grad.clone()
    xa.grad = None
    ((mean * gm.to(DEV)).sum() + (within * gw.to(DEV)).sum() + (between * gb.to(DEV)).sum()).backward()
    got = xa.grad.reshape(O, M, G, Sn, W).cpu().numpy().astype(np.float64)
    # float64 autograd of the same formulas
    x64t = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    mm_t = x64t.sum(3) / Sn
    vm_t = ((x64t - mm_t.unsqueeze(3)) ** 2).sum(3) / (Sn - 1)
    mu_t = mm_t.sum(1) / M
    wi_t = vm_t.sum(1) / M
    be_t = ((mm_t - mu_t.unsqueeze(1)) ** 2).sum(1) / (M - 1)
    ((mu_t * gm.double()).sum() + (wi_t * gw.double()).sum() + (be_t * gb.double()).sum()).backward()
    ref = x64t.grad.numpy()
    x64, mm, e_m, mu, e_mu = _fp64_parts(x)
    A = np.abs(gm.double().numpy()) / (M * Sn)
    Cw = 2 * np.abs(gw.double().numpy()) / ((Sn - 1) * M)
    Cb = 2 * np.abs(gb.double().numpy()) / ((M - 1) * Sn)
    A, Cw, Cb = (t[:, None, :, None, :] for t in (A, Cw, Cb))
    dx = np.abs(x64 - mm[:, :, :, None, :])
    am = np.abs(mm - mu[:, None])[:, :, :, None, :]
    em, emu = e_m[:, :, :, None, :], e_mu[:, None, :, None, :]
    mag = A + Cw * dx + Cb * am
    bound = 8 * U * mag + (1 + 8 * U) * (Cw * em + Cb * (em + emu)) + 1e-12 * mag
    err = np.abs(got - ref)
    print(f'ensemble_stats_backward {shape}: err / bound max {np.max(err / bound):.3f}')
    assert (err <= bound).all()
    # grad_mean alone is the constant g_mean / (M S) on every path, bit for bit as the kernel forms it
    want = torch.from_numpy((gm.numpy() / np.float32(M)) / np.float32(Sn)).to(DEV)      # (two IEEE float32 divisions, on the host)
    want = want[:, None, :, None, :].expand(O, M, G, Sn, W).reshape(O, M, G * Sn, W)
    assert torch.equal(g_mean_only, want)
    # NULL gradients through the entry point: each term alone, and their sum within the rounding of two float32 additions
    parts = [engine.ensemble_stats_backward(gm.to(DEV).contiguous() if k == 0 else None, gw.to(DEV).contiguous() if k == 1 else None,
                                            gb.to(DEV).contiguous() if k == 2 else None, xd, M, Sn) for k in range(3)]
    assert torch.equal(parts[0], want)
    total = sum(p.double() for p in parts).reshape(O, M, G, Sn, W).cpu().numpy()
    assert (np.abs(total - ref) <= bound + 4 * U * mag).all()


def test_on_a_real_solve_the_parts_are_finite_and_positive():
    from tests.test_gpu_ensemble_samples import M as MEM, SEED, TS, _members
    sdes, y0, model = _members(4, 17, 64)
    ts = torch.from_numpy(TS).to(DEV)
    with torch.no_grad():
        ys = S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0,
                               options={'seed': SEED, 'samples': 3, 'ensemble_samples': True, 'strict': True})
    mean, within, between = S.ensemble_stats(ys, MEM, 3)
    assert tuple(mean.shape) == (len(TS), 4, 64)
    assert torch.isfinite(mean).all() and torch.isfinite(within).all() and torch.isfinite(between).all()
    assert ((within + between) > 0).all() and (within[-1] > 0).all() and (between[-1] > 0).all()
    v = ys.double().reshape(len(TS), MEM, 4, 3, 64)
    assert torch.allclose(mean.double(), v.mean(dim=(1, 3)), rtol=0, atol=1e-5)
    assert torch.allclose(within.double(), v.var(dim=3).mean(dim=1), rtol=1e-4, atol=1e-9)
    assert torch.allclose(between.double(), v.mean(dim=3).var(dim=1), rtol=1e-4, atol=1e-9)
