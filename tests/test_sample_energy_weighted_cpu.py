"""The energy score of weighted, partially observed sample sets on the host: the entry points snsde_sample_energy_weighted /
_backward (declared, exported, bound, refusing bad arguments before a launch), and sample_energy(log_weight=, mask=) /
energy_loss(masked=True) on CPU tensors - the tensor-op statement - against the float64 numpy statement, autograd of the naive
pairwise statement, the unweighted function, replicated sets, the weighted CRPS at width 1, and the filtering recipe on
sdeint_filter.  No GPU compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine, train
from tests import sample_energy_weighted_reference as E
from tests.test_step_offset_cpu import Stub, _model

ERR_NULL, ERR_DIMS = -1, -2
INF, NAN = float('inf'), float('nan')
UNIT = 16 * 2.0 ** -53
NAMES = ('snsde_sample_energy_weighted', 'snsde_sample_energy_weighted_backward')
CPU_SHAPES = [(1, 2, 1), (3, 5, 3), (2, 40, 5), (2, 3, 17)]


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (14, 16)):
        assert f'SNSDE_API int {name}(' in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f' T {name}\n' in dyn
        assert len(getattr(lib, name).argtypes) == arity
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)
    assert S.sample_energy is engine.sample_energy and S.energy_loss is train.energy_loss


def _fwd(lib, outer=1, members=1, groups=1, samples=4, width=1, fair=1, path=0, nanm=0, ys=4096, target=4096, logw=4096, mask=4096, energy=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_energy_weighted(p(ys), p(target), p(logw), p(mask), outer, members, groups, samples, width, fair, path, nanm,
                                            p(energy), None)


def _bwd(lib, outer=1, members=1, groups=1, samples=4, width=1, fair=1, path=0, nanm=0, g=4096, ys=4096, target=4096, logw=4096, mask=4096,
         gys=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_energy_weighted_backward(p(g), p(ys), p(target), p(logw), p(mask), outer, members, groups, samples, width, fair,
                                                     path, nanm, p(gys), None, None)


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy non-null pointers: every case here must be refused before anything is launched."""
    lib = _lib.lib()
    for fn in (_fwd, _bwd):
        for path in (0, 1):
            for kw in (dict(), dict(logw=0), dict(mask=0), dict(logw=0, mask=0, nanm=1)):      # (both are nullable: never ERR_NULL)
                assert fn(lib, ys=0, path=path, **kw) == ERR_NULL and fn(lib, target=0, path=path, **kw) == ERR_NULL
                assert fn(lib, outer=0, path=path, **kw) == ERR_DIMS and fn(lib, members=0, path=path, **kw) == ERR_DIMS
                assert fn(lib, groups=0, path=path, **kw) == ERR_DIMS and fn(lib, samples=0, path=path, **kw) == ERR_DIMS
                assert fn(lib, width=0, path=path, **kw) == ERR_DIMS and fn(lib, groups=-3, path=path, **kw) == ERR_DIMS
                assert fn(lib, samples=257, path=path, **kw) == ERR_DIMS                                # N > 256
                assert fn(lib, samples=129, members=2, path=path, **kw) == ERR_DIMS                     # N = 258
                assert fn(lib, samples=1, members=1, fair=1, path=path, **kw) == ERR_DIMS               # fair with one sample
                assert fn(lib, groups=2 ** 62, width=8, path=path, **kw) == ERR_DIMS                    # 63-bit overflow
    assert _fwd(lib, energy=0) == ERR_NULL
    assert _bwd(lib, g=0) == ERR_NULL and _bwd(lib, gys=0) == ERR_NULL


def _t64(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a, np.float64)).requires_grad_(grad)


def _call(c, fair, grad=True, **kw):
    """sample_energy on the float64 copies of a reference case (G, N, V): energy, and with grad (grad_x, grad_y)."""
    G, N, V = c['x'].shape
    x, y = _t64(c['x'].reshape(G * N, V), grad), _t64(c['y'], grad)
    mask = None if c['obs'] is None else torch.from_numpy(c['obs'])
    e = S.sample_energy(x, N, y, fair=fair, log_weight=_t64(c['logw']), mask=mask, **kw)
    if not grad:
        return e
    gx, gy = torch.autograd.grad(e, (x, y), _t64(c['g']))
    return e.detach(), gx.reshape(G, N, V), gy


VARIANTS = [(None, True), (1.0, False), (1.0, True), (4.0, False), (4.0, True)]      # (log-weight scale, masked)


@pytest.mark.parametrize('variant', VARIANTS, ids=str)
@pytest.mark.parametrize('shape', CPU_SHAPES, ids=str)
def test_the_tensor_op_statement_against_the_numpy_statement(shape, variant):
    """Forward and autograd of the statement in float64, on float32 inputs with planted ties and NaN / Inf under the mask, within
    the reference's bounds at unit = 16 x 2^-53."""
    scale, masked = variant
    c = E.make_case(shape, scale, masked)
    for fair in (True, False):
        ref = E.energy(c['x'], c['y'], c['logw'], c['obs'], fair, c['g'], unit=UNIT)
        e, gx, gy = _call(c, fair)
        assert E.ratio(e.numpy(), ref['energy'], ref['E']) <= 1.0
        assert E.ratio(gx.numpy(), ref['grad_x'], ref['E_x']) <= 1.0 and E.ratio(gy.numpy(), ref['grad_y'], ref['E_y']) <= 1.0
        if masked:
            gap = ~c['obs']
            assert (gy.numpy()[gap] == 0).all() and (gx.numpy()[np.broadcast_to(gap[:, None], tuple(gx.shape))] == 0).all()


def _naive(x, y, logw, obs, fair):
    """The pairwise statement written out for one group: x (N, V), y (V,), obs (V,) bool, logw (N,) float64 tensors."""
    w = torch.softmax(logw, dim=0)
    D = (w * (1 - w)).sum() if fair else 1.0
    idx = torch.nonzero(obs)[:, 0]
    xo, yo = x[:, idx], y[idx]
    total = 0.0
    for n in range(x.shape[0]):
        total = total + w[n] * (xo[n] - yo).pow(2).sum().sqrt()
        for j in range(n + 1, x.shape[0]):
            total = total - w[n] * w[j] * (xo[n] - xo[j]).pow(2).sum().sqrt() / D
    return total


@pytest.mark.parametrize('fair', [True, False])
def test_value_and_gradients_equal_autograd_of_the_naive_pairwise_statement(fair):
    G, N, V = 3, 5, 4
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(G * N, V, generator=gen, dtype=torch.float64, requires_grad=True)
    y = torch.randn(G, V, generator=gen, dtype=torch.float64, requires_grad=True)
    logw = 2 * torch.randn(G, N, generator=gen, dtype=torch.float64)
    obs = torch.tensor([[1, 0, 1, 1], [1, 1, 1, 1], [0, 0, 1, 0]], dtype=torch.bool)
    e = S.sample_energy(x, N, y, fair=fair, log_weight=logw, mask=obs)
    want = torch.stack([_naive(x.reshape(G, N, V)[i], y[i], logw[i], obs[i], fair) for i in range(G)])
    assert float((e - want).detach().abs().max()) <= 1e-13
    ga, gb = torch.autograd.grad(e.sum(), (x, y)), torch.autograd.grad(want.sum(), (x, y))
    assert float((ga[0] - gb[0]).abs().max()) <= 1e-13 and float((ga[1] - gb[1]).abs().max()) <= 1e-13
    assert float(ga[0].reshape(G, N, V)[0, :, 1].abs().max()) == 0 and float(ga[1][2, 0].abs()) == 0


def test_equal_weights_and_a_mask_of_ones_are_the_unweighted_function():
    G, N, V = 4, 6, 5
    gen = torch.Generator().manual_seed(32)
    x = torch.randn(2, G * N, V, generator=gen, dtype=torch.float64)
    y = torch.randn(2, G, V, generator=gen, dtype=torch.float64)
    for fair in (True, False):
        for path in (False, True):
            want = engine.sample_energy_tensor_ops(x, N, y, fair, 1, path)
            lw = torch.full((G, N) if path else (2, G, N), -3.5, dtype=torch.float64)
            assert float((S.sample_energy(x, N, y, fair=fair, path=path, log_weight=lw) - want).abs().max()) <= 1e-13
            assert float((S.sample_energy(x, N, y, fair=fair, path=path, mask=torch.ones_like(y)) - want).abs().max()) <= 1e-13
            assert float((S.sample_energy(x, N, y, fair=fair, path=path, mask='nan') - want).abs().max()) <= 1e-13
    assert torch.isnan(S.sample_energy(x, N, torch.full_like(y, NAN))).all()      # (mask=None: a NaN target still poisons its row)


def test_integer_weights_are_the_replicated_set():
    G, N, V = 3, 4, 3
    counts = np.array([1, 3, 2, 1])
    c = E.make_case((G, N, V), ties=False)
    logw = torch.log(torch.tensor(counts, dtype=torch.float64)).expand(G, N)
    rep = E.replicate(c['x'], counts)
    x, xr, y = _t64(c['x'].reshape(G * N, V)), _t64(rep.reshape(G * rep.shape[1], V)), _t64(c['y'])
    got = S.sample_energy(x, N, y, fair=False, log_weight=logw)
    want = S.sample_energy(xr, int(counts.sum()), y, fair=False)
    assert float((got - want).abs().max()) <= 1e-13


def test_a_dead_sample_holding_nan_or_inf_is_the_set_without_it():
    G, N, V = 2, 5, 3
    c = E.make_case((G, N, V), 1.0)
    logw = c['logw'].astype(np.float64)
    logw[:, 3] = -INF
    x = c['x'].astype(np.float64)
    x[0, 3], x[1, 3] = NAN, INF
    keep = [0, 1, 2, 4]
    for fair in (True, False):
        xa, ya = _t64(x.reshape(G * N, V), True), _t64(c['y'], True)
        ea = S.sample_energy(xa, N, ya, fair=fair, log_weight=_t64(logw))
        xb, yb = _t64(x[:, keep].reshape(G * 4, V), True), _t64(c['y'], True)
        eb = S.sample_energy(xb, 4, yb, fair=fair, log_weight=_t64(logw[:, keep]))
        assert bool(torch.isfinite(ea).all()) and float((ea - eb).detach().abs().max()) <= 1e-13
        ga, gb = torch.autograd.grad(ea.sum(), (xa, ya)), torch.autograd.grad(eb.sum(), (xb, yb))
        gxa = ga[0].reshape(G, N, V)
        assert float(gxa[:, 3].abs().max()) == 0      # (its own row: an exact zero where it holds NaN)
        assert float((gxa[:, keep] - gb[0].reshape(G, 4, V)).abs().max()) <= 1e-13 and float((ga[1] - gb[1]).abs().max()) <= 1e-13


@pytest.mark.parametrize('bad', [[-INF] * 4, [0.0, NAN, 0.0, 0.0], [0.0, INF, 0.0, 0.0]], ids=['all-inf', 'nan', '+inf'])
def test_an_unusable_weight_row_is_nan_and_its_neighbours_are_unchanged(bad):
    G, N, V = 3, 4, 3
    c = E.make_case((G, N, V), 1.0, masked=True)
    for i in range(G):
        E.set_observed(c, i, 0, True)      # (every group has an observed column and a gap)
        E.set_observed(c, i, 1, False)
    logw = c['logw'].copy()
    clean = _call(dict(c, logw=logw), True)
    logw[1] = bad
    e, gx, gy = _call(dict(c, logw=logw), True)
    assert bool(torch.isnan(e[1])) and torch.equal(e[[0, 2]], clean[0][[0, 2]])
    assert torch.equal(gx[[0, 2]], clean[1][[0, 2]]) and torch.equal(gy[[0, 2]], clean[2][[0, 2]])
    obs = torch.from_numpy(c['obs'][1])
    assert bool(torch.isnan(gy[1][obs]).all()) and float(gy[1][~obs].abs().max()) == 0
    assert bool(torch.isnan(gx[1][:, obs]).all()) and float(gx[1][:, ~obs].abs().max()) == 0
    ref = E.energy(c['x'], c['y'], logw, c['obs'], True, c['g'], unit=UNIT)
    assert E.ratio(gx.numpy(), ref['grad_x'], ref['E_x']) <= 1.0 and E.ratio(e.numpy(), ref['energy'], ref['E']) <= 1.0


def test_one_live_sample_under_fair_is_nan_as_the_weighted_variance_is():
    x, y = torch.randn(3, 2, dtype=torch.float64, requires_grad=True), torch.randn(1, 2, dtype=torch.float64)
    lw = torch.tensor([[0.0, -INF, -INF]], dtype=torch.float64)
    e = S.sample_energy(x, 3, y, log_weight=lw)
    assert bool(torch.isnan(e).all())
    e0 = S.sample_energy(x, 3, y, fair=False, log_weight=lw)
    assert float((e0 - (x[0] - y[0]).norm()).detach().abs()) <= 1e-14
    gx, = torch.autograd.grad(e.sum(), x)
    assert bool(torch.isnan(gx[0]).all()) and float(gx[1:].abs().max()) == 0
    ref = E.energy(x.detach().numpy()[None], y.numpy(), lw.numpy(), None, True, np.ones(1))
    assert np.isnan(ref['energy']).all() and np.isnan(ref['grad_x'][0, 0]).all() and (ref['grad_x'][0, 1:] == 0).all()


def test_a_fully_masked_row_is_zero_with_zero_gradients_and_nothing_under_the_mask_is_read():
    G, N, V = 3, 4, 5
    c = E.make_case((G, N, V), 4.0, masked=True)
    c['obs'][1] = False
    c['x'][1], c['y'][1] = NAN, INF
    c['g'][2] = NAN                                       # (gaps get zeros by selection, whatever g is)
    E.set_observed(c, 2, 0, False)
    E.set_observed(c, 2, 1, True)
    E.set_observed(c, 0, 1, True)
    for fair in (True, False):
        e, gx, gy = _call(c, fair)
        assert float(e[1]) == 0 and float(gx[1].abs().max()) == 0 and float(gy[1].abs().max()) == 0
        assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(gx[0]).all()) and bool(torch.isfinite(gy[0]).all())
        gap = torch.from_numpy(~c['obs'])
        assert float(gy[gap].abs().max()) == 0 and float(gx[gap[:, None].expand_as(gx)].abs().max()) == 0
        assert bool(torch.isnan(gy[2][~gap[2]]).all())
        # the values under the mask do not matter, bit for bit
        c2 = dict(c, x=np.where(c['obs'][:, None], c['x'], 7.0).astype(np.float32), y=np.where(c['obs'], c['y'], -3.0).astype(np.float32))
        e2, gx2, gy2 = _call(c2, fair)
        assert torch.equal(e, e2) and torch.equal(gx[:2], gx2[:2]) and torch.equal(gy[:2], gy2[:2])


def test_mask_nan_is_the_explicit_mask_and_a_number_mask_is_a_flag():
    c = E.make_case((3, 5, 7), 1.0, masked=True)
    G, N, V = c['x'].shape
    x, y, lw = _t64(c['x'].reshape(G * N, V)), _t64(c['y']), _t64(c['logw'])
    obs = torch.from_numpy(c['obs'])
    want = S.sample_energy(x, N, y, log_weight=lw, mask=obs)
    assert torch.equal(S.sample_energy(x, N, y, log_weight=lw, mask='nan'), want)
    assert torch.equal(S.sample_energy(x, N, y, log_weight=lw, mask=obs.double() * 0.25), want)      # (fractional values do not weigh)
    assert torch.equal(S.sample_energy(x, N, y, log_weight=lw, mask=obs.float()), want)
    assert torch.equal(S.sample_energy(x, N, y, mask=obs.int()), S.sample_energy(x, N, y, mask=obs))


def test_path_mode_is_the_call_on_the_flattened_leading_axes():
    T_, G, N, W = 4, 3, 5, 2
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(T_, G * N, W, generator=gen, dtype=torch.float64, requires_grad=True)
    y = torch.randn(T_, G, W, generator=gen, dtype=torch.float64, requires_grad=True)
    lw = torch.randn(G, N, generator=gen, dtype=torch.float64)
    obs = torch.rand(T_, G, W, generator=gen) > 0.4
    e = S.sample_energy(x, N, y, path=True, log_weight=lw, mask=obs)
    ref = S.sample_energy(x.movedim(0, -2).reshape(G * N, T_ * W), N, y.movedim(0, -2).reshape(G, T_ * W), log_weight=lw,
                          mask=obs.movedim(0, -2).reshape(G, T_ * W))
    assert e.shape == (G,) and float((e - ref).detach().abs().max()) <= 1e-13
    ga, gb = torch.autograd.grad(e.sum(), (x, y)), torch.autograd.grad(ref.sum(), (x, y))
    assert float((ga[0] - gb[0]).abs().max()) <= 1e-13 and float((ga[1] - gb[1]).abs().max()) <= 1e-13
    # members pooled: the hand-pooled tensor
    M, Sn = 2, 3
    xm = torch.randn(T_, M, G * Sn, W, generator=gen, dtype=torch.float64)
    lm = torch.randn(T_, G, M * Sn, generator=gen, dtype=torch.float64)
    flat = xm.reshape(T_, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(T_, G * M * Sn, W)
    a = S.sample_energy(xm, Sn, y, members=M, log_weight=lm, mask=obs)
    assert a.shape == (T_, G) and torch.equal(a, S.sample_energy(flat, M * Sn, y, log_weight=lm, mask=obs))


def test_width_one_weighted_is_the_weighted_crps():
    G, N = 6, 9
    gen = torch.Generator().manual_seed(34)
    x = torch.randn(G * N, 1, generator=gen, dtype=torch.float64)
    x[1::N] = x[0::N]
    y, lw = torch.randn(G, 1, generator=gen, dtype=torch.float64), 2 * torch.randn(G, N, generator=gen, dtype=torch.float64)
    for fair in (True, False):
        e, c = S.sample_energy(x, N, y, fair=fair, log_weight=lw), S.sample_crps(x, N, y, fair=fair, log_weight=lw)[..., 0]
        assert float((e - c).abs().max()) <= 1e-12


def test_the_statement_slices_its_distance_plane_without_changing_a_value(monkeypatch):
    G, N, W = 7, 5, 3
    gen = torch.Generator().manual_seed(36)
    x, y, lw = torch.randn(2, G * N, W, generator=gen), torch.randn(2, G, W, generator=gen), torch.randn(2, G, N, generator=gen)
    obs = torch.rand(2, G, W, generator=gen) > 0.3
    whole = engine.sample_energy_weighted_tensor_ops(x, N, y, lw, obs)
    monkeypatch.setattr(engine, '_CDIST_MAX_PLANE', 3 * N * N)
    assert torch.equal(engine.sample_energy_weighted_tensor_ops(x, N, y, lw, obs), whole)


def test_argument_errors():
    x, y = torch.zeros(12, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match='log_weight has shape'):
        S.sample_energy(x, 3, y, log_weight=torch.zeros(4, 2))
    with pytest.raises(ValueError, match='log_weight has shape'):
        S.sample_energy(x.reshape(2, 6, 3), 3, y.reshape(2, 2, 3), path=True, log_weight=torch.zeros(2, 2, 3))      # (path: (B, N))
    with pytest.raises(ValueError, match='requires grad'):
        S.sample_energy(x, 3, y, log_weight=torch.zeros(4, 3, requires_grad=True))
    with pytest.raises(ValueError, match='floating-point'):
        S.sample_energy(x, 3, y, log_weight=torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match='mask has shape'):
        S.sample_energy(x, 3, y, mask=torch.ones(4, 2))
    with pytest.raises(ValueError, match="'nan'"):
        S.sample_energy(x, 3, y, mask='missing')
    with pytest.raises(ValueError, match='at least 2'):
        S.sample_energy(x, 1, torch.zeros(12, 3), mask='nan')
    assert S.sample_energy(torch.zeros(0, 3), 2, torch.zeros(0, 3), mask='nan').shape == (0,)


def test_energy_loss_masked_takes_nan_targets_and_value_mask_pairs():
    B, Sn, T_out, Cn = 3, 4, 5, 2
    gen = torch.Generator().manual_seed(35)
    pred = torch.randn(B * Sn, T_out, Cn, generator=gen, requires_grad=True)
    true = torch.randn(B, T_out, Cn, generator=gen)
    obs = torch.rand(B, T_out, Cn, generator=gen) > 0.4
    obs[1] = False                                                       # (a row with nothing observed adds 0)
    gaps = torch.where(obs, true, torch.full_like(true, NAN))
    loss = S.energy_loss(Sn, masked=True)(pred, gaps)
    want = S.sample_energy(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), mask=obs.reshape(B, -1)).mean()
    assert loss.shape == () and bool(torch.isfinite(loss)) and torch.equal(loss, want)
    assert torch.equal(S.energy_loss(Sn, masked=True)(pred, (true, obs)), want)
    assert torch.equal(S.energy_loss(Sn, masked=True)(pred, (true, obs.float())), want)
    assert torch.equal(S.energy_loss(Sn, masked=True)(pred, true), S.energy_loss(Sn)(pred, true))      # (no gap: the same score)
    loss.backward()
    g = pred.grad.reshape(B, Sn, T_out, Cn)
    assert bool(torch.isfinite(g).all()) and float(g[~obs[:, None].expand_as(g)].abs().max()) == 0 and float(g.abs().sum()) > 0
    assert bool(torch.isnan(S.energy_loss(Sn)(pred, gaps)))             # (the default is unchanged: a NaN target poisons the loss)
    with pytest.raises(ValueError, match='mask has shape'):
        S.energy_loss(Sn, masked=True)(pred, (true, obs[:, :2]))
    M = 2
    pm = torch.randn(M, B * Sn, T_out, Cn, generator=gen)
    assert torch.equal(S.energy_loss(Sn, members=M, masked=True)(pm, gaps),
                       S.sample_energy(pm.reshape(M, B * Sn, -1), Sn, true.reshape(B, -1), members=M, mask=obs.reshape(B, -1)).mean())


def test_a_train_loop_epoch_on_the_cpu_trains_on_a_target_with_gaps():
    torch.manual_seed(3)
    n, L, Cn, H, Sn = 8, 5, 2, 4, 3
    rng = np.random.default_rng(5)
    times = np.arange(L, dtype=np.float32)
    slope = rng.standard_normal((n, 1, Cn)).astype(np.float32) * 0.2
    X = slope * times[None, :, None] + 0.05 * rng.standard_normal((n, L, Cn)).astype(np.float32)
    X[:, :, 0] = times[None]
    y = np.stack([slope[:, 0, 1], -slope[:, 0, 1]], 1).astype(np.float32)
    y[::2, 0], y[3] = NAN, NAN                                           # gaps, and one row with nothing observed
    coeffs = torch.cat(S.controldiffeq.natural_cubic_spline_coeffs(torch.from_numpy(times), torch.from_numpy(X)), dim=-1)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(coeffs, torch.from_numpy(y), torch.full((n,), L - 1, dtype=torch.int64)),
                                         batch_size=n)
    model, field = S.make_sde_model('neurallsde', Cn, 2, H, H, 1)
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    kwargs = dict(method='euler', options={'seed': 1, 'samples': Sn, 'sample_grad': True})
    hist = train.train_loop(loader, loader, model, torch.from_numpy(times), opt, S.energy_loss(Sn, masked=True), 1, None, 'cpu', kwargs, 'valloss')
    assert len(hist) == 1 and np.isfinite(hist[0].train_metrics.loss) and hist[0].train_metrics.loss > 0
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


TS = torch.tensor([0.0, 0.75, 2.25, 4.0])


def _likelihood(k, yk):
    return -8.0 * (yk[:, :3] - 0.1 * k).pow(2).sum(-1).reshape(-1, 2)


@pytest.mark.parametrize('threshold', [0.0, 0.9])
def test_the_filtering_recipe_on_sdeint_filter(threshold):
    """sample_energy(filter_particles(r.ys, r.ancestor, S), S, target, log_weight=r.log_weight) on a short CPU run: at every time
    the weighted score of the explicitly resampled particles, by hand in float64."""
    m, pr = _model()
    y0, Sn = torch.from_numpy(pr['y0']), 2
    r = S.sdeint_filter(m, y0, TS, _likelihood, bm=Stub((8, 16)), method='euler', dt=0.25, options={'samples': Sn}, threshold=threshold,
                        generator=torch.Generator().manual_seed(5))
    T, B, H = r.ys.shape[0], r.ys.shape[1] // Sn, r.ys.shape[2]
    target = torch.randn(T, B, H, generator=torch.Generator().manual_seed(6))
    target[1, :, ::3] = NAN
    parts = S.filter_particles(r.ys, r.ancestor, Sn)
    for fair in (True, False):
        e = S.sample_energy(parts, Sn, target, fair=fair, log_weight=r.log_weight, mask='nan')
        assert tuple(e.shape) == (T, B)
        ref = E.energy(parts.reshape(T * B, Sn, H).numpy(), target.reshape(T * B, H).numpy(), r.log_weight.reshape(T * B, Sn).numpy(),
                       ~torch.isnan(target).reshape(T * B, H).numpy(), fair)
        assert E.ratio(e.reshape(-1).numpy(), ref['energy'], ref['E']) <= 1.0
        ep = S.sample_energy(parts, Sn, target, fair=fair, path=True, log_weight=r.log_weight[-1], mask='nan')
        assert tuple(ep.shape) == (B,) and bool(torch.isfinite(ep).all())
