"""Weighted sample sets on the host: the six entry points snsde_sample_{stats,crps,quantiles}_weighted[_backward] (declared,
exported, bound, validating before they launch), the tensor-op statements engine.sample_*_weighted_tensor_ops in float64 against the
numpy statement of tests/sample_weighted_reference.py and against autograd of a naive pairwise statement, the special values, the
argument errors, engine.filter_particles against a gather by hand, and the filtering recipe on torchsde.sdeint_filter with CPU
tensors.  No GPU compute.

Bounds: the statements run in float64 here, so the comparisons use the bounds of the reference with unit = 16 x 2^-53 (torch's
sums take another order than the kernels' chains and trees; a handful of roundings each)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests import sample_weighted_reference as R
from tests.test_step_offset_cpu import Stub, _model

ERR_NULL, ERR_DIMS = -1, -2
INF, NAN = float('inf'), float('nan')
UNIT = 16 * 2.0 ** -53
NAMES = ('snsde_sample_stats_weighted', 'snsde_sample_crps_weighted', 'snsde_sample_quantiles_weighted')
CPU_SHAPES = [(1, 1, 1), (1, 2, 1), (3, 5, 33), (2, 64, 7), (40, 3, 2)]


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    counts = dict(zip(NAMES, ((8, 10), (13, 13), (11, 12))))
    for name in NAMES:
        for full, n in zip((name, name + '_backward'), counts[name]):
            assert f'SNSDE_API int {full}(' in header
            assert full in _lib.EXPORTS and hasattr(lib, full)
            assert f' T {full}\n' in dyn
            assert len(getattr(lib, full).argtypes) == n, full
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)
    assert S.filter_particles is engine.filter_particles and S.torchsde.filter_particles is engine.filter_particles


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy non-null pointers: every case here must be refused before anything is launched."""
    lib = _lib.lib()
    p = lambda i: C.c_void_p(4096 * i)
    q = (C.c_float * 2)(0.25, 0.5)
    stats = lambda ys=p(1), lw=p(2), G=1, Sn=4, W=3, mean=p(3), var=p(4): lib.snsde_sample_stats_weighted(ys, lw, G, Sn, W, mean, var, None)
    assert stats(ys=None) == ERR_NULL and stats(lw=None) == ERR_NULL and stats(mean=None) == ERR_NULL
    assert stats(G=0) == ERR_DIMS and stats(Sn=257) == ERR_DIMS and stats(Sn=1) == ERR_DIMS and stats(W=0) == ERR_DIMS
    assert stats(G=1 << 62) == ERR_DIMS
    sb = lambda gm=p(1), gv=p(2), ys=p(3), lw=p(4), mean=p(5), Sn=4, out=p(6): lib.snsde_sample_stats_weighted_backward(gm, gv, ys, lw, mean, 1, Sn, 3, out, None)
    assert sb(gm=None) == ERR_NULL and sb(lw=None) == ERR_NULL and sb(out=None) == ERR_NULL and sb(ys=None) == ERR_NULL and sb(mean=None) == ERR_NULL
    assert sb(Sn=1) == ERR_DIMS and sb(Sn=300) == ERR_DIMS
    crps = lambda ys=p(1), y=p(2), lw=p(3), M=1, Sn=4, fair=1, out=p(4): lib.snsde_sample_crps_weighted(ys, y, lw, 1, M, 2, Sn, 3, fair, out, None, None, None)
    assert crps(ys=None) == ERR_NULL and crps(y=None) == ERR_NULL and crps(lw=None) == ERR_NULL and crps(out=None) == ERR_NULL
    assert crps(M=3, Sn=86) == ERR_DIMS and crps(Sn=1, fair=1) == ERR_DIMS and crps(Sn=0) == ERR_DIMS and crps(M=0) == ERR_DIMS
    cb = lambda g=p(1), ys=p(2), y=p(3), lw=p(4), Sn=4, fair=1, out=p(5): lib.snsde_sample_crps_weighted_backward(g, ys, y, lw, 1, 1, 2, Sn, 3, fair, out, None, None)
    assert cb(g=None) == ERR_NULL and cb(lw=None) == ERR_NULL and cb(out=None) == ERR_NULL and cb(Sn=1) == ERR_DIMS and cb(Sn=257) == ERR_DIMS
    quant = lambda ys=p(1), lw=p(2), Sn=4, n_q=2, qs=q, out=p(3): lib.snsde_sample_quantiles_weighted(ys, lw, 1, 1, 2, Sn, 3, n_q, qs, out, None)
    assert quant(ys=None) == ERR_NULL and quant(lw=None) == ERR_NULL and quant(out=None) == ERR_NULL and quant(qs=None) == ERR_NULL
    assert quant(n_q=0) == ERR_DIMS and quant(n_q=9, qs=(C.c_float * 9)()) == ERR_DIMS and quant(Sn=257) == ERR_DIMS
    for bad in (-0.1, 1.5, NAN):
        assert quant(qs=(C.c_float * 2)(0.5, bad)) == ERR_DIMS
    qb = lambda g=p(1), ys=p(2), lw=p(3), n_q=2, qs=q, out=p(4): lib.snsde_sample_quantiles_weighted_backward(g, ys, lw, 1, 1, 2, 4, 3, n_q, qs, out, None)
    assert qb(g=None) == ERR_NULL and qb(lw=None) == ERR_NULL and qb(out=None) == ERR_NULL and qb(n_q=9) == ERR_DIMS
    assert qb(qs=(C.c_float * 2)(2.0, 0.5)) == ERR_DIMS


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64)).requires_grad_(grad)


@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('shape', CPU_SHAPES, ids=str)
def test_the_tensor_op_statements_against_the_numpy_statement(shape, scale):
    """Forward and autograd of the three statements in float64, on the float32 inputs with planted ties, within the reference's
    bounds at unit = 16 x 2^-53; quantile gradients in the columns whose brackets are pinned."""
    G, N, W = shape
    c = R.make_case(shape, scale)
    lw, g, g2, gq = _t64(c['logw']), _t64(c['g']), _t64(c['g2']), _t64(c['gq'])
    var = N >= 2
    x = _t64(c['x'].reshape(G * N, W), True)
    mean, v = engine.sample_stats(x, N, var=var, log_weight=lw)
    gx, = torch.autograd.grad((mean * g).sum() + ((v * g2).sum() if var else 0.0), x)
    rs = R.stats(c['x'], c['logw'], c['g'], c['g2'] if var else None, unit=UNIT)
    ratios = dict(mean=R.ratio(mean.detach().numpy(), rs['mean'], rs['E_mean']),
                  stats_grad=R.ratio(gx.numpy().reshape(G, N, W), rs['grad'], rs['E_grad']))
    if var:
        ratios['var'] = R.ratio(v.detach().numpy(), rs['var'], rs['E_var'])
    for fair in ([True, False] if N >= 2 else [False]):
        y = _t64(c['y'], True)
        crps, rank, ties = engine.sample_crps(x, N, y, fair=fair, rank=True, log_weight=lw)
        cx, cy = torch.autograd.grad(crps, (x, y), g)
        rc = R.crps(c['x'], c['logw'], c['y'], fair, c['g'], unit=UNIT)
        ratios.update({f'crps[{fair}]': R.ratio(crps.detach().numpy(), rc['crps'], rc['E_crps']),
                       f'grad_x[{fair}]': R.ratio(cx.numpy().reshape(G, N, W), rc['grad_x'], rc['E_grad_x']),
                       f'grad_y[{fair}]': R.ratio(cy.numpy(), rc['grad_y'], rc['E_grad_y'])})
        assert rank.dtype == ties.dtype == torch.float32
        assert np.abs(rank.numpy() - rc['rank']).max() <= 2.0 ** -22 and np.abs(ties.numpy() - rc['ties']).max() <= 2.0 ** -22
    qv = engine.sample_quantiles(x, N, R.LEVELS, log_weight=lw)
    qx, = torch.autograd.grad(qv, x, gq)
    rq = R.quantiles(c['x'], c['logw'], R.LEVELS, c['gq'], unit=UNIT)
    cols = np.broadcast_to(rq['col_pinned'][:, None, :], (G, N, W))
    ratios['q'] = R.ratio(qv.detach().numpy(), rq['out'], rq['E'])
    ratios['q_grad'] = R.ratio(np.where(cols, qx.numpy().reshape(G, N, W), 0.0), np.where(cols, rq['grad'], 0.0), rq['E_grad'])
    share = 1.0 - float(rq['pinned'].mean())
    print(f'{shape} scale {scale}: err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()) + f'; brackets set aside {share:.4f}')
    assert max(ratios.values()) <= 1.0 and share <= R.SHARE_CAP, ratios


@pytest.mark.parametrize('shape', R.SHAPES + [R.POOLED], ids=str)
def test_the_reference_sets_aside_essentially_no_bracket_at_the_kernel_shapes(shape):
    """The condition the GPU test asserts, checked where the reference lives: at float32 round-off, with continuous random weights
    and the levels (0, 0.1, 0.5, 0.9, 1), the share of unpinned (level, group, column) entries stays within SHARE_CAP."""
    if len(shape) == 5:
        shape = (shape[0] * shape[2], shape[1] * shape[3], shape[4])
    for scale in R.SCALES:
        c = R.make_case(shape, scale)
        share = 1.0 - float(R.quantiles(c['x'], c['logw'])['pinned'].mean())
        print(f'{shape} scale {scale}: brackets set aside {share:.5f}')
        assert share <= R.SHARE_CAP


def test_crps_and_its_gradients_equal_autograd_of_the_pairwise_statement():
    """crps = E_w |X - y| - sum_ij w_i w_j |x_i - x_j| / (2 D) written with the (N, N) term, differentiated by autograd: the statement
    from a sort and the closed-form adjoint of the reference agree with it, ties included (sign(0) = 0 on both sides)."""
    shape = (3, 5, 4)
    G, N, W = shape
    c = R.make_case(shape, 1.0)
    w = torch.softmax(_t64(c['logw']), dim=-1)[:, :, None]
    for fair in (True, False):
        x, y = _t64(c['x'], True), _t64(c['y'], True)
        D = (w * (1 - w)).sum(1) if fair else 1.0
        pair = (w[:, :, None] * w[:, None, :] * (x[:, :, None] - x[:, None, :]).abs()).sum((1, 2))
        naive = (w * (x - y[:, None]).abs()).sum(1) - pair / (2 * D)
        nx, ny = torch.autograd.grad(naive, (x, y), _t64(c['g']))
        x2, y2 = _t64(c['x'].reshape(G * N, W), True), _t64(c['y'], True)
        got = engine.sample_crps_weighted_tensor_ops(x2, N, y2, _t64(c['logw']), fair)
        gx, gy = torch.autograd.grad(got, (x2, y2), _t64(c['g']))
        assert torch.allclose(got, naive, rtol=1e-12, atol=1e-13)
        assert torch.allclose(gx.reshape(G, N, W), nx, rtol=1e-11, atol=1e-13) and torch.allclose(gy, ny, rtol=1e-11, atol=1e-12)
        r = R.crps(c['x'], c['logw'], c['y'], fair, c['g'])
        assert np.allclose(r['grad_x'], nx.numpy(), rtol=1e-11, atol=1e-13) and np.allclose(r['grad_y'], ny.numpy(), rtol=1e-11, atol=1e-12)


def test_statistics_equal_autograd_of_the_plain_weighted_estimators():
    shape = (3, 5, 4)
    G, N, W = shape
    c = R.make_case(shape, 4.0)
    w = torch.softmax(_t64(c['logw']), dim=-1)[:, :, None]
    x = _t64(c['x'], True)
    mean = (w * x).sum(1)
    var = (w * (x - mean[:, None]) ** 2).sum(1) / (1 - (w * w).sum(1))      # (1 - sum w^2 = sum w (1 - w))
    nx, = torch.autograd.grad((mean * _t64(c['g'])).sum() + (var * _t64(c['g2'])).sum(), x)
    r = R.stats(c['x'], c['logw'], c['g'], c['g2'])
    assert np.allclose(r['mean'], mean.detach().numpy(), rtol=1e-12) and np.allclose(r['var'], var.detach().numpy(), rtol=1e-9)
    assert np.allclose(r['grad'], nx.numpy(), rtol=1e-9, atol=1e-12)


def test_equal_weights_are_the_unweighted_functions_and_torch_quantile():
    shape = (3, 7, 5)
    G, N, W = shape
    c = R.make_case(shape, 1.0)
    x, y, zero = _t64(c['x'].reshape(G * N, W)), _t64(c['y']), torch.zeros(G, N, dtype=torch.float64)
    m0, v0 = engine.sample_stats(x, N)
    m1, v1 = engine.sample_stats(x, N, log_weight=zero)
    assert torch.allclose(m0, m1, rtol=1e-13) and torch.allclose(v0, v1, rtol=1e-12)
    for fair in (True, False):
        a, ra, ta = engine.sample_crps(x, N, y, fair=fair, rank=True)
        b, rb, tb = engine.sample_crps(x, N, y, fair=fair, rank=True, log_weight=zero)
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-14) and torch.allclose(ra / N, rb) and torch.allclose(ta / N, tb)
    levels = (0.0, 0.1, 0.5, 0.9, 1.0)
    want = torch.quantile(x.reshape(G, N, W), torch.tensor(levels, dtype=torch.float64), dim=1)
    got = engine.sample_quantiles(x, N, levels, log_weight=zero)
    gap = float((x.max() - x.min()))
    assert float((got - want).abs().max()) <= 2.0 ** -22 * (N - 1) * gap      # (the levels are rounded to float32)


def test_dead_samples_and_unusable_weight_sets_in_the_statements():
    shape = (3, 5, 4)
    G, N, W = shape
    c = R.make_case(shape, 1.0)
    x, logw = c['x'].copy(), c['logw'].copy()
    x[:, 3, 0::2], x[:, 3, 1::2] = NAN, INF
    logw[:, 3] = -INF
    logw[1, 4] = logw[1].max() - 800.0      # (float64 exp underflows: dead as well)
    xs = _t64(x.reshape(G * N, W), True)
    y = _t64(c['y'], True)
    lw = _t64(logw)
    mean, var = engine.sample_stats(xs, N, log_weight=lw)
    crps = engine.sample_crps(xs, N, y, log_weight=lw)
    qv = engine.sample_quantiles(xs, N, R.LEVELS, log_weight=lw)
    gx, = torch.autograd.grad(mean.sum() + var.sum() + crps.sum() + qv.sum(), xs)
    gx = gx.reshape(G, N, W)
    assert bool(torch.isfinite(mean).all() and torch.isfinite(var).all() and torch.isfinite(crps).all() and torch.isfinite(qv).all())
    assert bool((gx[:, 3] == 0).all()) and bool((gx[1, 4] == 0).all()) and bool(torch.isfinite(gx).all())
    keep = [0, 1, 2, 4]
    r = R.stats(x[:, keep], logw[:, keep])
    assert np.allclose(mean.detach().numpy(), r['mean'], rtol=1e-12) and np.allclose(var.detach().numpy(), r['var'], rtol=1e-10)
    assert np.allclose(qv.detach().numpy(), R.quantiles(x[:, keep], logw[:, keep])['out'], rtol=1e-12)
    assert np.allclose(crps.detach().numpy(), R.crps(x[:, keep], logw[:, keep], c['y'], True)['crps'], rtol=1e-10, atol=1e-13)
    # unusable weight sets: NaN in the group, in every output and gradient element, and nowhere else
    for bad in ('all', NAN, INF):
        lw2 = c['logw'].astype(np.float64).copy()
        if bad == 'all':
            lw2[1] = -INF
        else:
            lw2[1, 2] = bad
        xs = _t64(c['x'].reshape(G * N, W), True)
        y = _t64(c['y'], True)
        outs = list(engine.sample_stats(xs, N, log_weight=_t64(lw2))) + list(engine.sample_crps(xs, N, y, rank=True, log_weight=_t64(lw2)))
        outs.append(engine.sample_quantiles(xs, N, R.LEVELS, log_weight=_t64(lw2)))
        for o in outs:
            o = o if o.dim() == 2 else o.movedim(0, -1)
            assert bool(torch.isnan(o[1]).all()) and bool(torch.isfinite(o[[0, 2]]).all()), bad
        for o in (outs[0], outs[1], outs[2], outs[5]):
            gx, = torch.autograd.grad(o.sum(), xs, retain_graph=True)
            gx = gx.reshape(G, N, W)
            assert bool(torch.isnan(gx[1]).all()) and bool(torch.isfinite(gx[[0, 2]]).all()), bad
    # one live sample: the mean is that sample, the variance and the fair score 0 / 0
    one = torch.tensor([[0.0, -INF, -INF]], dtype=torch.float64)
    xs = torch.tensor([[1.5], [NAN], [2.0]], dtype=torch.float64)
    mean, var = engine.sample_stats(xs, 3, log_weight=one)
    assert float(mean) == 1.5 and bool(torch.isnan(var))
    assert bool(torch.isnan(engine.sample_crps(xs, 3, torch.zeros(1, 1, dtype=torch.float64), log_weight=one)))
    assert float(engine.sample_crps(xs, 3, torch.zeros(1, 1, dtype=torch.float64), fair=False, log_weight=one)) == 1.5
    assert engine.sample_quantiles(xs, 3, (0.0, 0.3, 1.0), log_weight=one).flatten().tolist() == [1.5, 1.5, 1.5]
    # a live NaN: every level of its column is NaN
    xs = torch.tensor([[1.5, 1.0], [NAN, 2.0], [2.0, 3.0]], dtype=torch.float64)
    qv = engine.sample_quantiles(xs, 3, (0.0, 0.5), log_weight=torch.zeros(1, 3, dtype=torch.float64))
    assert bool(torch.isnan(qv[:, 0, 0]).all()) and qv[:, 0, 1].tolist() == [1.0, 2.0]


def test_weighted_quantiles_by_hand():
    """Weights (0.5, 0.25, 0.25) on x = (10, 30, 20): ranks 0, 2, 1; nodes p = 0, 1 and, for x = 20, A / (1 - w) = 0.5 / 0.75 = 2 / 3.
    q = 1 / 3 is half-way from 10 to 20; q = 5 / 6 half-way from 20 to 30.  A zero-weight sample between two live ones moves nothing."""
    lw = torch.log(torch.tensor([[0.5, 0.25, 0.25]], dtype=torch.float64))
    xs = torch.tensor([[10.0], [30.0], [20.0]], dtype=torch.float64)
    qv = engine.sample_quantiles(xs, 3, (0.0, 0.5, 1.0), log_weight=lw).flatten()
    assert torch.allclose(qv, torch.tensor([10.0, 17.5, 30.0], dtype=torch.float64), rtol=1e-7)
    lw4 = torch.cat((lw, torch.tensor([[-INF]], dtype=torch.float64)), dim=1)
    xs4 = torch.cat((xs, torch.tensor([[15.0]], dtype=torch.float64)))
    assert torch.equal(engine.sample_quantiles(xs4, 4, (0.0, 0.5, 1.0), log_weight=lw4).flatten(), qv)


def test_argument_errors():
    x, y = torch.zeros(6, 3), torch.zeros(2, 3)
    lw = torch.zeros(2, 3)
    with pytest.raises(ValueError, match='log_weight has shape'):
        engine.sample_stats(x, 3, log_weight=torch.zeros(3, 2))
    with pytest.raises(ValueError, match='log_weight has shape'):
        engine.sample_crps(x, 3, y, log_weight=torch.zeros(2, 4))
    with pytest.raises(ValueError, match='log_weight has shape'):
        engine.sample_quantiles(x.reshape(2, 3, 3), 3, [0.5], members=2, log_weight=torch.zeros(1, 3))
    with pytest.raises(ValueError, match='floating-point'):
        engine.sample_quantiles(x, 3, [0.5], log_weight=torch.zeros(2, 3, dtype=torch.int64))
    for call in (lambda w: engine.sample_stats(x, 3, log_weight=w), lambda w: engine.sample_crps(x, 3, y, log_weight=w),
                 lambda w: engine.sample_quantiles(x, 3, [0.5], log_weight=w)):
        with pytest.raises(ValueError, match='requires grad'):
            call(lw.clone().requires_grad_(True))
        with torch.no_grad():
            call(lw.clone().requires_grad_(True))      # (nothing is recorded: fine)
    with pytest.raises(ValueError, match='at least 2'):
        engine.sample_crps(torch.zeros(2, 3), 1, y, log_weight=torch.zeros(2, 1))
    with pytest.raises(ValueError, match='samples >= 2'):
        engine.sample_stats(torch.zeros(2, 3), 1, log_weight=torch.zeros(2, 1))
    with pytest.raises(ValueError, match=r'in \[0, 1\]'):
        engine.sample_quantiles(x, 3, [1.5], log_weight=lw)
    with pytest.raises(ValueError, match='target has shape'):
        engine.sample_crps(x, 3, torch.zeros(3, 3), log_weight=lw)
    # log_weight=None is the code path of before: the same objects come back from the same calls
    assert torch.equal(engine.sample_crps(x + 1, 3, y, log_weight=None), engine.sample_crps(x + 1, 3, y))
    # more than 256 pooled samples take the statement, on any device
    big = torch.randn(300, 2, generator=torch.Generator().manual_seed(0))
    m, _ = engine.sample_stats(big, 300, log_weight=torch.zeros(1, 300))
    assert torch.allclose(m, big.mean(0, keepdim=True), atol=1e-6)


def test_filter_particles_against_a_gather_by_hand():
    T, B, Sn, H = 3, 2, 4, 5
    gen = torch.Generator().manual_seed(3)
    ys = torch.randn(T, B * Sn, H, generator=gen)
    anc = torch.randint(0, Sn, (T, B, Sn), generator=gen, dtype=torch.int32)
    out = engine.filter_particles(ys, anc, Sn)
    for k in range(T):
        for b in range(B):
            for j in range(Sn):
                assert torch.equal(out[k, b * Sn + j], ys[k, b * Sn + int(anc[k, b, j])])
    ident = torch.arange(Sn, dtype=torch.int32).expand(T, B, Sn)
    assert torch.equal(engine.filter_particles(ys, ident, Sn), ys)
    assert torch.equal(engine.filter_particles(ys[0], anc[0], Sn), out[0])
    with pytest.raises(ValueError, match='ancestor must be'):
        engine.filter_particles(ys, anc.float(), Sn)
    with pytest.raises(ValueError, match='ancestor must be'):
        engine.filter_particles(ys, anc[:, :, :2], Sn)
    with pytest.raises(ValueError, match='whole number'):
        engine.filter_particles(ys, anc, 3)


TS = torch.tensor([0.0, 0.75, 2.25, 4.0])


def _likelihood(k, yk):
    return -8.0 * (yk[:, :3] - 0.1 * k).pow(2).sum(-1).reshape(-1, 2)


@pytest.mark.parametrize('threshold', [0.0, 0.9, 1.0])
def test_the_filtering_recipe_on_sdeint_filter(threshold):
    """sample_stats(filter_particles(r.ys, r.ancestor, S), S, log_weight=r.log_weight) on a short CPU run: at every time it is the
    weighted mean of the explicitly resampled particles - the same weights, the same gather, by hand."""
    m, pr = _model()
    y0, Sn = torch.from_numpy(pr['y0']), 2
    r = S.sdeint_filter(m, y0, TS, _likelihood, bm=Stub((8, 16)), method='euler', dt=0.25, options={'samples': Sn}, threshold=threshold,
                        generator=torch.Generator().manual_seed(5))
    mean, var = S.sample_stats(S.filter_particles(r.ys, r.ancestor, Sn), Sn, log_weight=r.log_weight)
    T, B, H = r.ys.shape[0], r.ys.shape[1] // Sn, r.ys.shape[2]
    assert tuple(mean.shape) == (T, B, H) == tuple(var.shape)
    for k in range(T):
        for b in range(B):
            parts = torch.stack([r.ys[k, b * Sn + int(r.ancestor[k, b, j])] for j in range(Sn)]).double()
            w = torch.softmax(r.log_weight[k, b].double(), dim=-1)[:, None]
            want = (w * parts).sum(0)
            assert torch.allclose(mean[k, b].double(), want, rtol=1e-5, atol=1e-6)
            wv = (w * (parts - want) ** 2).sum(0) / (w * (1 - w)).sum()
            assert torch.allclose(var[k, b].double(), wv, rtol=1e-4, atol=1e-6)
    if threshold >= 1.0:      # (resampled at every step: equal weights, the plain statistics of the gathered particles)
        m0, _ = S.sample_stats(S.filter_particles(r.ys, r.ancestor, Sn), Sn)
        assert torch.allclose(mean[1:], m0[1:], rtol=1e-5, atol=1e-6)
