"""The statistics and score kernels on NaN, +-Inf, signed zeros and degenerate sample sets (tests/score_special_cases.py holds
the inputs, the float64 references and the contract).  For every function, forward and backward, at every layout of a shape:

  forward      every output element has the class (finite, +Inf, -Inf, NaN) of the float64 reference, and lies within the
               function's existing error bound where that class is finite; rank and ties are the exact integers;
  backward     on the sets whose forward value is finite - all-equal sets, sets on the observation, +0 / -0 mixtures, duplicated
               extremes among them - the documented formula within the existing gradient bound, exact zeros where it is zero;
               on the other sets the values are not prescribed;
  run-to-run   a second launch gives the same result everywhere, special sets included;
  isolation    the same call with the special sets replaced by clean values gives, bit for bit, the same outputs and gradients
               in every set that was clean in both: nothing of a special set reaches a neighbour through LDS rows, exchange
               areas, butterfly sums or the grid stride.

Shapes (G, N, W): (1, 2, 3) - two of the four waves of a score workgroup hold no sample, and the exchange rows >= N of the
quantile kernel were never staged; (2, 5, 70) - uneven quarters, two column tiles, a tail tile with six live lanes;
(2, 17, 5) - past the minimum LDS rows; (1, 256, 4) - the LDS cap, the last NaN at sample 255; (8200, 3, 2) - tiles t and
t + 8192 share a workgroup: specials in groups 5 and 6, isolation on groups 8197 and 8198; the energy score adds (2, 5, 17),
the special component one past a chunk of 16; ensemble statistics and the pooled scores run at (outer, M, G, S, W) =
(2, 3, 2, 4, 6) with the special samples in member 1."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from tests import score_special_cases as C

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
U = C.U


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # (a copy: the fixtures are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """Equal after nan_to_num to three distinct sentinels, equal NaN masks - and, beyond that, equal bits wherever no NaN stands
    (a +0 against a -0 differs)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ka = dict(nan=1.25e30, posinf=2.5e30, neginf=-5e30)
    ok = ~np.isnan(a)
    return np.array_equal(np.nan_to_num(a, **ka), np.nan_to_num(b, **ka)) and np.array_equal(a.view(np.int32)[ok], b.view(np.int32)[ok])


def _forward(what, got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    cg, cr = C.classes(got), C.classes(ref)
    assert np.array_equal(cg, cr), (what, np.argwhere(cg != cr)[:4].tolist(), got[cg != cr][:4], ref[cg != cr][:4])
    fin = cr == C.FINITE
    err, b = np.abs(got[fin] - ref[fin]), np.broadcast_to(bound, ref.shape)[fin]
    assert (err <= b).all(), (what, float(np.max(err - b)))


def _backward(what, got, ref, bound, finite_sets, zeros=True):
    """finite_sets: a mask, broadcast over got, of the elements whose set has a finite forward value."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = np.broadcast_to(finite_sets, got.shape)
    assert np.isfinite(ref[m]).all() and np.isfinite(got[m]).all(), what
    assert (np.abs(got[m] - ref[m]) <= np.broadcast_to(bound, got.shape)[m]).all(), what
    if zeros:
        assert (got[m][ref[m] == 0] == 0).all(), what


def _contract(runs, keeps, big=False):
    """runs = (first, second, clean): dicts name -> array of one call each; keeps: name -> mask of the elements whose set is
    clean.  Run-to-run on everything, isolation on the clean sets."""
    first, second, clean = runs
    for name in first:
        assert _same(first[name], second[name]), ('run-to-run', name)
        keep = np.broadcast_to(keeps[name], first[name].shape)
        assert keep.any() or first[name].shape[0] == 1
        assert _same(first[name][keep], clean[name][keep]), ('isolation', name)
        if big:      # the tiles that share a workgroup with the special ones through the grid stride
            assert keep[8197:8199].all() and _same(first[name][8197:8199], clean[name][8197:8199]), ('isolation at t + 8192', name)


def _cases(shape, vector=False, span=None):
    for layout in range(C.layouts(shape, vector)):
        yield C.build(shape, layout, vector, True, span), C.build(shape, layout, vector, False, span)


# ---- sample_stats ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', C.SHAPES)
def test_sample_stats(shape):
    G, N, W = shape
    gm, gv = C.upstream(shape, 2)

    def run(x):
        xd = _dev(x).reshape(G * N, W).requires_grad_(True)
        mean, var = S.sample_stats(xd, N)
        assert 'SampleStats' in type(mean.grad_fn).__name__
        gx, = torch.autograd.grad([mean, var], xd, [_dev(gm), _dev(gv)])
        plain = S.sample_stats(xd.detach(), N)      # (no autograd node: the same kernel)
        assert _same(_np(plain[0]), _np(mean)) and _same(_np(plain[1]), _np(var))
        return dict(mean=_np(mean), var=_np(var), gx=_np(gx).reshape(G, N, W))

    for (x, y, pat), (xc, yc, _) in _cases(shape):
        r = C.ref_sample_stats(x, gm, gv)
        runs = run(x), run(x), run(xc)
        _forward('mean', runs[0]['mean'], r['mean'], r['e_m'])
        _forward('var', runs[0]['var'], r['var'], r['bound_v'])
        fin = np.isfinite(r['mean']) & np.isfinite(r['var'])
        _backward('grad_ys', runs[0]['gx'], r['gx'], r['gx_bound'], fin[:, None], zeros=False)
        keep = pat == C.CLEAN
        _contract(runs, dict(mean=keep, var=keep, gx=keep[:, None]), big=G > 8)


# ---- sample_crps -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fair', [True, False])
@pytest.mark.parametrize('shape', C.SHAPES)
def test_sample_crps(shape, fair):
    G, N, W = shape
    g, = C.upstream(shape, 1)

    def run(x, y):
        xd, yd = _dev(x).reshape(G * N, W).requires_grad_(True), _dev(y).requires_grad_(True)
        crps, rank, ties = S.sample_crps(xd, N, yd, fair=fair, rank=True)
        assert type(crps.grad_fn).__name__.startswith('_SampleCRPS')
        gx, gy = torch.autograd.grad(crps, (xd, yd), _dev(g))
        return dict(crps=_np(crps), rank=_np(rank), ties=_np(ties), gx=_np(gx).reshape(G, N, W), gy=_np(gy))

    for (x, y, pat), (xc, yc, _) in _cases(shape):
        r = C.ref_crps(x, y, fair, g)
        runs = run(x, y), run(x, y), run(xc, yc)
        _forward('crps', runs[0]['crps'], r['crps'], (2 * N + 4) * U * r['scale'])
        assert np.array_equal(runs[0]['rank'], r['rank'].astype(np.float32)) and np.array_equal(runs[0]['ties'], r['ties'].astype(np.float32))
        fin = np.isfinite(r['crps'])
        _backward('grad_ys', runs[0]['gx'], r['gx'], 4 * U * r['gx_scale'], fin[:, None])
        _backward('grad_target', runs[0]['gy'], r['gy'], r['gy_bound'], fin)
        keep = pat == C.CLEAN
        _contract(runs, dict(crps=keep, rank=keep, ties=keep, gx=keep[:, None], gy=keep), big=G > 8)


# ---- sample_quantiles --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', C.SHAPES)
def test_sample_quantiles(shape):
    """Before the kernel flagged the NaNs of a column, a level whose rank no sample held read an exchange row nobody had written
    (a staged sample, or at N < 16 whatever the LDS held) and the level k = 0 raced between the minimum and the NaN.  Measured
    on an MI355X with the library of the commit before the flag, this test failed at all five shapes: at (1, 2, 3) the set
    [NaN, 4.2574] gave 3.3119 at level 1 in one launch and 1.6441 in the next; at (2, 17, 5) sets with a NaN gave -2.1098,
    -2.3405, 0.7883, 0.6281 where NaN is due; at (2, 5, 70) and (1, 256, 4) level 0 of a set with a NaN came out NaN in one
    launch and -1.2350 / -6.0700 (the minimum) in the next; [1, NaN, 3, 2, 5] gave [NaN, 3, 5] at levels (0, 0.5, 1)."""
    G, N, W = shape
    Q = len(C.QS)
    gq = np.stack(C.upstream(shape, Q, seed=11))

    def run(x):
        xd = _dev(x).reshape(G * N, W).requires_grad_(True)
        out = S.sample_quantiles(xd, N, C.QS)
        assert type(out.grad_fn).__name__.startswith('_SampleQuantiles')
        gx, = torch.autograd.grad(out, xd, _dev(gq))
        assert _same(_np(S.sample_quantiles(xd.detach(), N, C.QS)), _np(out))
        return dict(out=_np(out), gx=_np(gx).reshape(G, N, W))

    with_nan = 0
    for (x, y, pat), (xc, yc, _) in _cases(shape):
        r = C.ref_quantiles(x)
        runs = run(x), run(x), run(xc)
        print(f'sample_quantiles {shape}: sets with a NaN {int(r["bad"].sum())}, of which all levels NaN '
              f'{int(np.isnan(runs[0]["out"][:, r["bad"]]).all(0).sum())}')
        _forward('quantiles', runs[0]['out'], r['out'], 3 * U * r['scale'])
        assert np.isnan(runs[0]['out'][:, r['bad']]).all()
        with_nan += int(r['bad'].sum())
        # each term g (1 - frac) or g frac is a rounded difference and a rounded product, a sample adds at most 2 Q of them
        want, mag = C.ref_quantiles_grad(r, gq)
        fin = np.isfinite(r['out']).all(0)
        _backward('grad_ys', runs[0]['gx'], want, (2 * Q + 2) * U * mag, fin[:, None])
        keep = pat == C.CLEAN
        _contract(runs, dict(out=keep[None], gx=keep[:, None]), big=False)
        if G > 8:
            assert keep[8197:8199].all()
            assert _same(runs[0]['out'][:, 8197:8199], runs[2]['out'][:, 8197:8199]) and _same(runs[0]['gx'][8197:8199], runs[2]['gx'][8197:8199])
    assert with_nan >= 3      # (nan_first, nan_last and all_nan were planted)


def test_the_quantiles_of_a_set_with_a_nan_are_nan_whichever_wave_holds_it():
    """x = [1, NaN, 3, 2, 5]: the permutation ranks used to be [0, 0, 2, 1, 3], samples 0 and 1 in different waves' quarters."""
    x = torch.tensor([1.0, float('nan'), 3.0, 2.0, 5.0], device=DEV).reshape(5, 1)
    for _ in range(3):
        assert bool(torch.isnan(S.sample_quantiles(x, 5, (0.0, 0.5, 1.0))).all())
    for at in range(5):      # the NaN in every quarter
        v = torch.tensor([1.0, 4.0, 3.0, 2.0, 5.0], device=DEV)
        v[at] = float('nan')
        assert bool(torch.isnan(S.sample_quantiles(v.reshape(5, 1), 5, C.QS)).all()), at
    v = torch.tensor([1.0, float('nan'), 3.0, 2.0, 5.0], device=DEV).reshape(5, 1).requires_grad_(True)
    ga, = torch.autograd.grad(S.sample_quantiles(v, 5, (0.0, 0.5, 1.0)), v, torch.ones(3, 1, 1, device=DEV))
    gb, = torch.autograd.grad(S.sample_quantiles(v, 5, (0.0, 0.5, 1.0)), v, torch.ones(3, 1, 1, device=DEV))
    # the documented backward of such a set: the NaN sample gets an exact zero, the four finite ones rank among themselves
    # (1 < 2 < 3 < 5: ranks 0, 2, 1, 3) and hold k = 0 and k = 2; nobody holds k = 4
    assert torch.equal(ga, gb) and ga.flatten().tolist() == [1.0, 0.0, 1.0, 0.0, 0.0]


# ---- sample_energy -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', [False, True])
@pytest.mark.parametrize('fair', [True, False])
@pytest.mark.parametrize('shape', C.ENERGY_SHAPES)
def test_sample_energy(shape, fair, path):
    G, N, W = shape
    g, = C.upstream(shape, 1, vector=True)

    def run(x, y):
        xd, yd = _dev(x).reshape(G * N, W).requires_grad_(True), _dev(y).requires_grad_(True)
        e = S.sample_energy(xd, N, yd, fair=fair, path=path)
        assert type(e.grad_fn).__name__.startswith('_SampleEnergy') and tuple(e.shape) == (G,)
        gx, gy = torch.autograd.grad(e, (xd, yd), _dev(g))
        return dict(energy=_np(e), gx=_np(gx).reshape(G, N, W), gy=_np(gy))

    for (x, y, pat), (xc, yc, _) in _cases(shape, vector=True):
        r = C.ref_energy(x, y, fair, g)
        runs = run(x, y), run(x, y), run(xc, yc)
        _forward('energy', runs[0]['energy'], r['energy'], (W / 2 + 2 * N + 8) * U * r['scale'])
        fin = np.isfinite(r['energy'])
        _backward('grad_ys', runs[0]['gx'], r['gx'], r['gx_bound'], fin[:, None, None])
        _backward('grad_target', runs[0]['gy'], r['gy'], r['gy_bound'], fin[:, None])
        keep = pat == C.CLEAN
        _contract(runs, dict(energy=keep, gx=keep[:, None, None], gy=keep[:, None]), big=G > 8)


# ---- the ensemble layout: the member stride is part of the addressing ---------------------------------------------------------------

def _ensemble_cases():
    O, M, G, Sn, W = C.ENSEMBLE
    return _cases((O * G, M * Sn, W), span=(Sn, 2 * Sn))


def _pool(t5):
    """(O, M, G, S, W) -> the pooled sets (O G, M S, W)."""
    O, M, G, Sn, W = C.ENSEMBLE
    return np.ascontiguousarray(t5.reshape(O, M, G, Sn, W).transpose(0, 2, 1, 3, 4)).reshape(O * G, M * Sn, W)


def test_ensemble_stats():
    O, M, G, Sn, W = C.ENSEMBLE
    gm, gw, gb = (a.reshape(O, G, W) for a in C.upstream((O * G, M * Sn, W), 3))

    def run(x):
        xd = _dev(C.to_members(x, O, M, Sn)).reshape(O, M, G * Sn, W).requires_grad_(True)
        mean, within, between = S.ensemble_stats(xd, M, Sn)
        assert type(mean.grad_fn).__name__ == '_EnsembleStatsBackward'
        gx, = torch.autograd.grad([mean, within, between], xd, [_dev(gm), _dev(gw), _dev(gb)])
        return dict(mean=_np(mean), within=_np(within), between=_np(between), gx=_np(gx).reshape(O, M, G, Sn, W))

    for (x, y, pat), (xc, yc, _) in _ensemble_cases():
        r = C.ref_ensemble_stats(C.to_members(x, O, M, Sn), gm, gw, gb)
        runs = run(x), run(x), run(xc)
        _forward('mean', runs[0]['mean'], r['mean'], r['e_mu'])
        _forward('within', runs[0]['within'], r['within'], r['bound_w'])
        _forward('between', runs[0]['between'], r['between'], r['bound_b'])
        fin = np.isfinite(r['mean']) & np.isfinite(r['within']) & np.isfinite(r['between'])
        _backward('grad_ys', runs[0]['gx'], r['gx'], r['gx_bound'], fin[:, None, :, None, :], zeros=False)
        keep = (pat == C.CLEAN).reshape(O, G, W)
        _contract(runs, dict(mean=keep, within=keep, between=keep, gx=keep[:, None, :, None, :]))


@pytest.mark.parametrize('fair', [True, False])
def test_pooled_scores_of_an_ensemble(fair):
    O, M, G, Sn, W = C.ENSEMBLE
    N, Q = M * Sn, len(C.QS)
    pooled = (O * G, N, W)
    g, = C.upstream(pooled, 1)
    gq = np.stack(C.upstream(pooled, Q, seed=11))

    def run(x, y):
        xd = _dev(C.to_members(x, O, M, Sn)).reshape(O, M, G * Sn, W).requires_grad_(True)
        yd = _dev(y).reshape(O, G, W).requires_grad_(True)
        crps, rank, ties = S.sample_crps(xd, Sn, yd, fair=fair, members=M, rank=True)
        out = S.sample_quantiles(xd, Sn, C.QS, members=M)
        assert type(crps.grad_fn).__name__.startswith('_SampleCRPS') and type(out.grad_fn).__name__.startswith('_SampleQuantiles')
        gx, gy = torch.autograd.grad(crps, (xd, yd), _dev(g).reshape(O, G, W))
        hx, = torch.autograd.grad(out, xd, _dev(gq).reshape(Q, O, G, W))
        return dict(crps=_np(crps).reshape(O * G, W), rank=_np(rank).reshape(O * G, W), ties=_np(ties).reshape(O * G, W),
                    gx=_pool(_np(gx)), gy=_np(gy).reshape(O * G, W), out=_np(out).reshape(Q, O * G, W), hx=_pool(_np(hx)))

    for (x, y, pat), (xc, yc, _) in _ensemble_cases():
        r, rq = C.ref_crps(x, y, fair, g), C.ref_quantiles(x)
        runs = run(x, y), run(x, y), run(xc, yc)
        _forward('crps', runs[0]['crps'], r['crps'], (2 * N + 4) * U * r['scale'])
        assert np.array_equal(runs[0]['rank'], r['rank'].astype(np.float32)) and np.array_equal(runs[0]['ties'], r['ties'].astype(np.float32))
        fin = np.isfinite(r['crps'])
        _backward('grad_ys', runs[0]['gx'], r['gx'], 4 * U * r['gx_scale'], fin[:, None])
        _backward('grad_target', runs[0]['gy'], r['gy'], r['gy_bound'], fin)
        _forward('quantiles', runs[0]['out'], rq['out'], 3 * U * rq['scale'])
        want, mag = C.ref_quantiles_grad(rq, gq)
        _backward('quantile grad_ys', runs[0]['hx'], want, (2 * Q + 2) * U * mag, np.isfinite(rq['out']).all(0)[:, None])
        keep = pat == C.CLEAN
        _contract(runs, dict(crps=keep, rank=keep, ties=keep, gx=keep[:, None], gy=keep, out=keep[None], hx=keep[:, None]))


@pytest.mark.parametrize('path', [False, True])
def test_pooled_energy_of_an_ensemble(path):
    """path: the vector of a group is (outer, W), so the special pseudo-groups (o, g) of the fixture join: the reference is formed
    on the permuted (G, N, outer W) copy."""
    O, M, G, Sn, W = C.ENSEMBLE
    N = M * Sn
    pooled = (O * G, N, W)
    g, = C.upstream(pooled, 1, vector=True)
    g = g[:G] if path else g

    def views(x, y, pat):
        if not path:
            return x, y, pat == C.CLEAN
        xp = np.ascontiguousarray(x.reshape(O, G, N, W).transpose(1, 2, 0, 3)).reshape(G, N, O * W)
        return xp, np.ascontiguousarray(y.reshape(O, G, W).transpose(1, 0, 2)).reshape(G, O * W), (pat.reshape(O, G) == C.CLEAN).all(0)

    def joined(t):      # gradients (O G, .., W) in the layout of `views`: the outer axis joins the last
        if not path:
            return t
        t = t.reshape((O, G) + t.shape[1:])
        return np.ascontiguousarray(np.moveaxis(t, 0, -2)).reshape(t.shape[1:-1] + (O * W,))

    def run(x, y):
        xd = _dev(C.to_members(x, O, M, Sn)).reshape(O, M, G * Sn, W).requires_grad_(True)
        yd = _dev(y).reshape(O, G, W).requires_grad_(True)
        e = S.sample_energy(xd, Sn, yd, members=M, path=path)
        assert type(e.grad_fn).__name__.startswith('_SampleEnergy')
        gx, gy = torch.autograd.grad(e, (xd, yd), _dev(g).reshape(e.shape))
        return dict(energy=_np(e).reshape(-1), gx=joined(_pool(_np(gx))), gy=joined(_np(gy).reshape(O * G, W)))

    for (x, y, pat), (xc, yc, _) in _cases(pooled, vector=True, span=(Sn, 2 * Sn)):
        xv, yv, keep = views(x, y, pat)
        V = xv.shape[-1]
        r = C.ref_energy(xv, yv, True, g)
        runs = run(x, y), run(x, y), run(xc, yc)
        _forward('energy', runs[0]['energy'], r['energy'], (V / 2 + 2 * N + 8) * U * r['scale'])
        fin = np.isfinite(r['energy'])
        _backward('grad_ys', runs[0]['gx'], r['gx'], r['gx_bound'], fin[:, None, None])
        _backward('grad_target', runs[0]['gy'], r['gy'], r['gy_bound'], fin[:, None])
        _contract(runs, dict(energy=keep, gx=keep[:, None, None], gy=keep[:, None]))


# ---- the tensor-op routes on the GPU: N = 257, nine levels ---------------------------------------------------------------------------

def test_tensor_op_routes_obey_the_forward_class_contract():
    shape = (2, 257, 3)
    G, N, W = shape
    nine = tuple(i / 8 for i in range(9))
    for vector in (False, True):
        for (x, y, pat), _ in _cases(shape, vector):
            xd, yd = _dev(x).reshape(G * N, W).requires_grad_(True), _dev(y)
            for fair in (True, False):
                if vector:
                    r = C.ref_energy(x, y, fair)
                    e = S.sample_energy(xd, N, yd, fair=fair)
                    assert not type(e.grad_fn).__name__.startswith('_SampleEnergy')
                    _forward('energy', _np(e), r['energy'], (W / 2 + 2 * N + 8) * U * r['scale'])
                else:
                    r = C.ref_crps(x, y, fair)
                    crps, rank, ties = S.sample_crps(xd, N, yd, fair=fair, rank=True)
                    assert not type(crps.grad_fn).__name__.startswith('_SampleCRPS')
                    _forward('crps', _np(crps), r['crps'], (2 * N + 4) * U * r['scale'])
                    assert np.array_equal(_np(rank), r['rank'].astype(np.float32)) and np.array_equal(_np(ties), r['ties'].astype(np.float32))
            if not vector:
                rq = C.ref_quantiles(x)
                out = S.sample_quantiles(xd, N, C.QS)
                assert not type(out.grad_fn).__name__.startswith('_SampleQuantiles')
                _forward('quantiles', _np(out), rq['out'], 3 * U * rq['scale'])
    small = (2, 5, 70)
    for (x, y, pat), _ in _cases(small):
        xd = _dev(x).reshape(10, 70).requires_grad_(True)
        rq = C.ref_quantiles(x, nine)
        out = S.sample_quantiles(xd, 5, nine)
        assert not type(out.grad_fn).__name__.startswith('_SampleQuantiles')
        _forward('nine levels', _np(out), rq['out'], 3 * U * rq['scale'])
