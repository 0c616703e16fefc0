"""tests/score_special_cases.py on the CPU: its float64 references against independent statements, the premises of its fixture,
and the forward class contract on the tensor-op routes (CPU float32 and float64) of the five functions."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests import score_special_cases as C

SMALL = [(1, 2, 3), (2, 5, 70), (2, 17, 5)]


def _each(shape, vector=False):
    for layout in range(C.layouts(shape, vector)):
        yield C.build(shape, layout, vector)


def _agree(got, ref, tol, what):
    """The same class everywhere, and |got - ref| <= tol where the class is finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(C.classes(got), C.classes(ref)), what
    fin = np.isfinite(ref)
    assert (np.abs(got[fin] - ref[fin]) <= np.broadcast_to(tol, ref.shape)[fin]).all(), what


@pytest.mark.parametrize('shape', SMALL)
def test_stats_reference_is_torch_mean_and_var(shape):
    G, N, W = shape
    for x, y, pat in _each(shape):
        r = C.ref_sample_stats(x)
        t = torch.from_numpy(x.copy()).double()
        _agree(r['mean'], t.mean(1).numpy(), 1e-13, 'mean')
        _agree(r['var'], t.var(1).numpy(), 1e-12, 'var')
    x5 = C.to_members(C.build((4, 12, 6), 0, span=(4, 8))[0], 2, 3, 4)
    r = C.ref_ensemble_stats(x5)
    t = torch.from_numpy(x5).double()
    _agree(r['mean'], t.mean(3).mean(1).numpy(), 1e-13, 'ensemble mean')
    _agree(r['within'], t.var(3).mean(1).numpy(), 1e-12, 'within')
    _agree(r['between'], t.mean(3).var(1).numpy(), 1e-12, 'between')


@pytest.mark.parametrize('shape', SMALL)
def test_quantile_reference_against_torch_quantile(shape):
    """Clean sets: every level.  Sets with an infinity: the levels whose two neighbouring order statistics are finite
    (torch.quantile interpolates by lerp(x_(k), x_(k+1), frac) even at frac = 0, so an infinite neighbour it does not need turns
    its value into NaN; the formula of `sample_quantiles` reads x_(k) alone there).  Sets with a NaN: NaN at every level, as
    torch.quantile gives."""
    G, N, W = shape
    seen = set()
    for x, y, pat in _each(shape):
        r = C.ref_quantiles(x)
        tq = torch.quantile(torch.from_numpy(x.copy()).double(), torch.tensor(C.QS, dtype=torch.float64), dim=1).numpy()
        srt = np.sort(x.astype(np.float64), axis=1)
        bad = np.isnan(x).any(1)
        for i, k in enumerate(r['ks']):
            both = np.isfinite(srt[:, k]) & np.isfinite(srt[:, min(k + 1, N - 1)]) & ~bad
            assert (np.abs(r['out'][i][both] - tq[i][both]) <= 1e-6).all()      # (frac is rounded to float32 on one side only)
            assert both[(pat == C.CLEAN)].all()
        assert np.isnan(r['out'][:, bad]).all() and np.isnan(tq[:, bad]).all() and not np.isnan(r['out'][:, ~bad & np.isfinite(x).all(1)]).any()
        seen |= {C.PATTERNS[p] for p in pat[bad]}
        inf_set = np.isinf(x).any(1) & ~bad      # the formula on infinities: the extremes are the infinities themselves
        assert (r['out'][0][inf_set] == x.min(1)[inf_set]).all() and (r['out'][-1][inf_set] == x.max(1)[inf_set]).all()
    assert seen == {'nan_first', 'nan_last', 'all_nan'}


@pytest.mark.parametrize('fair', [True, False])
@pytest.mark.parametrize('shape', SMALL)
def test_score_references_against_the_float64_tensor_op_statements(shape, fair):
    G, N, W = shape
    for x, y, pat in _each(shape):
        r = C.ref_crps(x, y, fair)
        xt, yt = torch.from_numpy(x.copy()).double().reshape(G * N, W), torch.from_numpy(y.copy()).double()
        crps, rank, ties = engine.sample_crps_tensor_ops(xt, N, yt, fair=fair, rank=True)
        _agree(crps.numpy(), r['crps'], 1e-12, 'crps')
        assert np.array_equal(rank.numpy(), r['rank']) and np.array_equal(ties.numpy(), r['ties'])
    for shape_e in (shape, (2, 5, 17)):
        Ge, Ne, We = shape_e
        for x, y, pat in _each(shape_e, True):
            r = C.ref_energy(x, y, fair)
            xt, yt = torch.from_numpy(x.copy()).double().reshape(Ge * Ne, We), torch.from_numpy(y.copy()).double()
            _agree(engine.sample_energy_tensor_ops(xt, Ne, yt, fair=fair).numpy(), r['energy'], 1e-12, 'energy')


def test_gradient_references_against_float64_autograd_on_finite_sets():
    shape = (2, 5, 70)
    G, N, W = shape
    x, y, pat = C.build(shape, 0)
    g, g2 = C.upstream(shape, 2)
    xt, yt = torch.from_numpy(x.copy()).double().requires_grad_(True), torch.from_numpy(y.copy()).double().requires_grad_(True)
    r = C.ref_crps(x, y, True, g)
    fin = np.isfinite(r['crps'])
    crps = engine.sample_crps_tensor_ops(xt.reshape(G * N, W), N, yt)
    gx, gy = torch.autograd.grad(crps[torch.from_numpy(fin)], (xt, yt), torch.from_numpy(g.astype(np.float64))[torch.from_numpy(fin)])
    fx = np.broadcast_to(fin[:, None], x.shape)
    assert np.allclose(gx.numpy()[fx], r['gx'][fx], rtol=0, atol=1e-12) and np.allclose(gy.numpy()[fin], r['gy'][fin], rtol=0, atol=1e-12)
    assert {'all_equal', 'all_equal_obs', 'signed_zeros', 'dup_extremes'} <= {C.PATTERNS[p] for p in pat[fin & (pat >= 0)]}
    rs = C.ref_sample_stats(x, g, g2)
    fs = np.isfinite(rs['mean']) & np.isfinite(rs['var'])
    m, v = xt.sum(1) / N, None
    v = ((xt - m.unsqueeze(1)) ** 2).sum(1) / (N - 1)
    sel = torch.from_numpy(fs)
    gs, = torch.autograd.grad((m * torch.from_numpy(g).double())[sel].sum() + (v * torch.from_numpy(g2).double())[sel].sum(), xt)
    fsx = np.broadcast_to(fs[:, None], x.shape)
    assert np.allclose(gs.numpy()[fsx], rs['gx'][fsx], rtol=0, atol=1e-12)
    # the energy score: per group
    for layout in range(C.layouts((2, 5, 17), True)):
        xe, ye, pe = C.build((2, 5, 17), layout, True)
        ge, = C.upstream((2, 5, 17), 1, True)
        re = C.ref_energy(xe, ye, True, ge)
        fe = np.isfinite(re['energy'])
        xt, yt = torch.from_numpy(xe.copy()).double().requires_grad_(True), torch.from_numpy(ye.copy()).double().requires_grad_(True)
        e = engine.sample_energy_tensor_ops(xt.reshape(10, 17), 5, yt)
        gx, gy = torch.autograd.grad(e[torch.from_numpy(fe)], (xt, yt), torch.from_numpy(ge.astype(np.float64))[torch.from_numpy(fe)])
        assert np.allclose(gx.numpy()[fe], re['gx'][fe], rtol=0, atol=1e-12) and np.allclose(gy.numpy()[fe], re['gy'][fe], rtol=0, atol=1e-12)
        if C.PATTERNS[pe[0]] in ('all_equal_obs', 'signed_zeros'):
            assert fe[0] and not re['gx'][0].any() and not re['gy'][0].any()


@pytest.mark.parametrize('shape', C.ENERGY_SHAPES)
def test_fixture_premises(shape):
    """Every pattern is planted in every shape and next to clean sets; only the slots differ from the clean tensors; every
    finite reference value is below 1e6; and the references of a shape show every class the functions can produce: all four
    among the means and the quantiles, finite and NaN for the variance, the CRPS (an infinite |d| meets an infinite c d) and
    the energy score, which also reaches +Inf under an infinite observation - so no check passes because nothing was special."""
    G, N, W = shape
    for vector in (False, True):
        planted, cls = set(), {k: set() for k in ('mean', 'var', 'quantiles', 'crps', 'energy')}
        for layout in range(C.layouts(shape, vector)):
            x, y, pat = C.build(shape, layout, vector)
            xc, yc, patc = C.build(shape, layout, vector, special=False)
            planted |= {C.PATTERNS[p] for p in pat.ravel() if p >= 0}
            assert np.isfinite(xc).all() and np.isfinite(yc).all() and np.array_equal(pat, patc)
            assert (pat == C.CLEAN).any() or (vector and G == 1)      # (one group: the energy score has no neighbour there)
            keep = (pat == C.CLEAN)[:, None] if not vector else (pat == C.CLEAN)[:, None, None]
            keep = np.broadcast_to(keep, x.shape)
            assert np.array_equal(x[keep].view(np.int32), xc[keep].view(np.int32))
            ky = np.broadcast_to((pat == C.CLEAN) if not vector else (pat == C.CLEAN)[:, None], y.shape)
            assert np.array_equal(y[ky].view(np.int32), yc[ky].view(np.int32))
            if G > 8:
                assert set(np.argwhere(pat >= 0)[:, 0]) == set(C.BIG_GROUPS)
            vals = []
            if not vector:
                s, q = C.ref_sample_stats(x), C.ref_quantiles(x)
                vals += [('mean', s['mean']), ('var', s['var']), ('quantiles', q['out'])]
            for fair in (True, False):
                vals += [('energy', C.ref_energy(x, y, fair)['energy'])] if vector else [('crps', C.ref_crps(x, y, fair)['crps'])]
            for name, v in vals:
                cls[name] |= set(np.unique(C.classes(v)).tolist())
                assert (np.abs(v[np.isfinite(v)]) < 1e6).all()
        assert planted == set(C.PATTERNS)
        if vector:
            assert cls['energy'] == {C.FINITE, C.POS_INF, C.NAN}
        else:
            assert cls['mean'] == cls['quantiles'] == {C.FINITE, C.POS_INF, C.NEG_INF, C.NAN}
            assert cls['var'] == cls['crps'] == {C.FINITE, C.NAN}


def test_ensemble_fixture_plants_in_member_one():
    O, M, G, Sn, W = C.ENSEMBLE
    for layout in range(C.layouts((O * G, M * Sn, W))):
        x, y, pat = C.build((O * G, M * Sn, W), layout, span=(Sn, 2 * Sn))
        x5 = C.to_members(x, O, M, Sn)
        assert x5.shape == C.ENSEMBLE
        assert np.isfinite(x5[:, 0]).all() or 'all_nan' in {C.PATTERNS[p] for p in pat.ravel() if p >= 0}
        single = np.isin(pat, [C.PATTERNS.index(n) for n in ('nan_first', 'nan_last', 'pos_inf', 'neg_inf', 'both_inf', 'two_pos_inf')])
        member1 = ~np.isfinite(x5[:, 1]).all(2).reshape(O * G, W)      # (O, G, S, W) -> a non-finite value somewhere in member 1
        assert (member1[single]).all() and np.isfinite(x5[:, 2].reshape(O * G, Sn, W).transpose(0, 2, 1)[single]).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('shape', SMALL)
def test_tensor_op_routes_obey_the_forward_class_contract(shape, dtype):
    """CPU tensors take the tensor-op route of every function: the class of every output element is the reference's, and finite
    values agree with it within the float32 bounds (float64: far inside them)."""
    G, N, W = shape
    for x, y, pat in _each(shape):
        xt, yt = torch.from_numpy(x.copy()).to(dtype).reshape(G * N, W), torch.from_numpy(y.copy()).to(dtype)
        s = C.ref_sample_stats(x)
        mean, var = S.sample_stats(xt, N)
        _agree(mean.numpy(), s['mean'], s['e_m'], 'mean')
        _agree(var.numpy(), s['var'], s['bound_v'], 'var')
        q = C.ref_quantiles(x)
        _agree(S.sample_quantiles(xt, N, C.QS).numpy(), q['out'], 3 * C.U * q['scale'], 'quantiles')
        for fair in (True, False):
            r = C.ref_crps(x, y, fair)
            crps, rank, ties = S.sample_crps(xt, N, yt, fair=fair, rank=True)
            _agree(crps.numpy(), r['crps'], (2 * N + 4) * C.U * r['scale'], 'crps')
            assert np.array_equal(rank.numpy(), r['rank']) and np.array_equal(ties.numpy(), r['ties'])
    for x, y, pat in _each(shape, True):
        xt, yt = torch.from_numpy(x.copy()).to(dtype).reshape(G * N, W), torch.from_numpy(y.copy()).to(dtype)
        for fair in (True, False):
            for path in (False, True):
                r = C.ref_energy(x, y, fair)
                _agree(S.sample_energy(xt, N, yt, fair=fair, path=path).numpy(), r['energy'], (W / 2 + 2 * N + 8) * C.U * r['scale'], 'energy')
    O, M, Ge, Sn, We = C.ENSEMBLE
    for layout in range(C.layouts((O * Ge, M * Sn, We))):
        x5 = C.to_members(C.build((O * Ge, M * Sn, We), layout, span=(Sn, 2 * Sn))[0], O, M, Sn)
        r = C.ref_ensemble_stats(x5)
        mean, within, between = S.ensemble_stats(torch.from_numpy(x5).to(dtype).reshape(O, M, Ge * Sn, We), M, Sn)
        _agree(mean.numpy(), r['mean'], r['e_mu'], 'ensemble mean')
        _agree(within.numpy(), r['within'], r['bound_w'], 'within')
        _agree(between.numpy(), r['between'], r['bound_b'], 'between')


def test_the_issue_example_on_the_tensor_op_route():
    x = torch.tensor([1.0, float('nan'), 3.0, 2.0, 5.0]).reshape(5, 1)
    assert bool(torch.isnan(S.sample_quantiles(x, 5, (0.0, 0.5, 1.0))).all())
    clean = torch.tensor([1.0, 4.0, 3.0, 2.0, 5.0]).reshape(5, 1)
    assert S.sample_quantiles(clean, 5, (0.0, 0.5, 1.0)).flatten().tolist() == [1.0, 3.0, 5.0]
