"""snsde_sample_energy_weighted and its adjoint on the GPU, through sample_energy(log_weight=, mask=).

Shapes (scores, N, V) are the small shapes of the unweighted GPU test (tests/sample_energy_weighted_reference.py: SHAPES): N on
either side of each bucket edge 39 | 40, 87 | 88, 151 | 152, N + 1 rows either side of a row block (64 | 65), a chunk boundary with
one live tail column (V = 65), nine chunks (V = 130), the cap N = 256 (the 156 KB of the backward), and the smallest fair score;
one pooled `members` layout and one path=True case whose chunks of 16 columns cross the outer axis.  Log-weights N(0, 1) and
N(0, 16), each with and without a mask of about 40 % gaps whose ys / target entries hold NaN / Inf; and the mask alone.

Forward and both gradients against the float64 numpy statement, inside the first-order bounds that module derives from the
documented summation order (nothing measured, no entry set aside); the worst ratio of every shape is printed.  The float64
references are computed once per case from the float32 inputs and shared."""
import functools

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests import sample_energy_weighted_reference as E
from tests.buffer_arena import FILLS, Arena, place, recorded_calls, replay, same_bits
from tests.helpers import make_problem
from tests.kernel_cases import STEP_OFFSET_CASES

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
INF, NAN = float('inf'), float('nan')
VARIANTS = [(1.0, False), (4.0, False), (1.0, True), (4.0, True), (None, True)]      # (log-weight scale, masked)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(shape, scale, masked):
    """Inputs with planted ties and everything the float64 statement gives for them, both values of fair.  Never modified."""
    c = E.make_case(shape, scale, masked)
    for fair in (True, False):
        c[fair] = E.energy(c['x'], c['y'], c['logw'], c['obs'], fair, c['g'])
    return c


def _run(c, fair, **kw):
    """sample_energy and both gradients on the device for a reference case (G, N, V)."""
    G, N, V = c['x'].shape
    xd, yd = _dev(c['x']).reshape(G * N, V).requires_grad_(True), _dev(c['y']).requires_grad_(True)
    e = S.sample_energy(xd, N, yd, fair=fair, log_weight=_dev(c['logw']), mask=_dev(c['obs']), **kw)
    assert type(e.grad_fn).__name__.startswith('_SampleEnergyWeighted')
    gx, gy = torch.autograd.grad(e, (xd, yd), _dev(c['g']))
    return e.detach(), gx.reshape(G, N, V), gy


@pytest.mark.parametrize('variant', VARIANTS, ids=str)
@pytest.mark.parametrize('shape', E.SHAPES, ids=str)
def test_forward_and_gradients_against_float64(shape, variant):
    """energy within E, every component of grad_ys within E_x and of grad_target within E_y (the reference's docstring derives the
    three); exact zeros at the gaps; two launches give the same bits."""
    c = _case(shape, *variant)
    worst = {}
    for fair in (True, False):
        r = c[fair]
        e, gx, gy = _run(c, fair)
        assert tuple(e.shape) == (shape[0],) and e.dtype == torch.float32
        worst[fair] = (E.ratio(e.cpu().numpy(), r['energy'], r['E']), E.ratio(gx.cpu().numpy(), r['grad_x'], r['E_x']),
                       E.ratio(gy.cpu().numpy(), r['grad_y'], r['E_y']))
        e2, gx2, gy2 = _run(c, fair)
        assert same_bits(e, e2) and same_bits(gx, gx2) and same_bits(gy, gy2)
        if c['obs'] is not None:
            gap = _dev(~c['obs'])
            assert bool((gy[gap] == 0).all()) and bool((gx[gap[:, None].expand_as(gx)] == 0).all())
    print(f'sample_energy_weighted {shape} {variant}: err / bound (energy, grad_ys, grad_target) fair {worst[True][0]:.3f} {worst[True][1]:.3f} '
          f'{worst[True][2]:.3f}, unfair {worst[False][0]:.3f} {worst[False][1]:.3f} {worst[False][2]:.3f}')
    assert max(max(v) for v in worst.values()) <= 1.0, worst


def _pool_ref(x, y, logw, obs, g, O, M, G, Sn, W, path, fair):
    """The float64 statement of an (O, M, G Sn, W) layout: pooled by hand, path -> the outer axis joins the vector."""
    N = M * Sn
    xp = x.reshape(O, M, G, Sn, W).transpose(0, 2, 1, 3, 4).reshape(O, G, N, W)
    if path:
        return E.energy(xp.transpose(1, 2, 0, 3).reshape(G, N, O * W), y.transpose(1, 0, 2).reshape(G, O * W), logw,
                        None if obs is None else obs.transpose(1, 0, 2).reshape(G, O * W), fair, g)
    return E.energy(xp.reshape(O * G, N, W), y.reshape(O * G, W), None if logw is None else logw.reshape(O * G, N),
                    None if obs is None else obs.reshape(O * G, W), fair, g.reshape(O * G))


@pytest.mark.parametrize('path', [False, True], ids=['members pooled', 'path across the outer axis'])
def test_pooled_members_and_path_mode_against_float64(path):
    """outer = 3, M = 2, W = 33: under path V = 99 and the chunks of 16 columns cross o at 33 and 66; the members axis is
    addressing only.  Gradients are compared in the layout of ys."""
    O, M, G, Sn, W = 3, 2, 4, 3, 33
    N = M * Sn
    rng = np.random.default_rng(12)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, y = f(O, M, G * Sn, W), f(O, G, W)
    x[:, 1, 0::Sn] = x[:, 0, 1::Sn]      # coincident samples across members
    logw, g = 2 * f(*((G, N) if path else (O, G, N))), f(*((G,) if path else (O, G)))
    obs = rng.random((O, G, W)) >= E.MASK_SHARE
    x = np.where(np.repeat(obs, Sn, axis=1)[:, None], x, np.nan).astype(np.float32)
    y = np.where(obs, y, np.nan).astype(np.float32)
    for fair in (True, False):
        r = _pool_ref(x, y, logw, obs, g, O, M, G, Sn, W, path, fair)
        xd, yd = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
        e = S.sample_energy(xd, Sn, yd, fair=fair, members=M, path=path, log_weight=_dev(logw), mask='nan')
        assert tuple(e.shape) == ((G,) if path else (O, G))
        gx, gy = torch.autograd.grad(e, (xd, yd), _dev(g))
        gxp = gx.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G, N, W)
        if path:
            gxp, gyp = gxp.permute(1, 2, 0, 3).reshape(G, N, O * W), gy.permute(1, 0, 2).reshape(G, O * W)
        else:
            gxp, gyp = gxp.reshape(O * G, N, W), gy.reshape(O * G, W)
        ratios = (E.ratio(e.detach().reshape(-1).cpu().numpy(), r['energy'], r['E']), E.ratio(gxp.cpu().numpy(), r['grad_x'], r['E_x']),
                  E.ratio(gyp.cpu().numpy(), r['grad_y'], r['E_y']))
        print(f'sample_energy_weighted pooled path={path} fair={fair}: err / bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}')
        assert max(ratios) <= 1.0, ratios
        assert bool(torch.equal(e.detach(), S.sample_energy(xd.detach(), Sn, yd.detach(), fair=fair, members=M, path=path, log_weight=_dev(logw),
                                                            mask=_dev(obs))))      # (mask='nan' is the explicit mask, bit for bit)


def test_unaligned_and_non_contiguous_inputs_give_the_bits_of_their_clones():
    G, N, W = 4, 6, 37
    gen = torch.Generator().manual_seed(2)
    buf, tb, lb, mb = (torch.randn(n + 1, generator=gen).to(DEV) for n in (G * N * W, G * W, G * N, G * W))
    mb = (mb > -0.3).float()
    g = torch.randn(G, generator=gen).to(DEV)
    xu, tu = buf[1:].reshape(G * N, W).requires_grad_(True), tb[1:].reshape(G, W).requires_grad_(True)      # 4 bytes off a 16-byte boundary
    xc, tc = buf[1:].clone().reshape(G * N, W).requires_grad_(True), tb[1:].clone().reshape(G, W).requires_grad_(True)
    a = S.sample_energy(xu, N, tu, log_weight=lb[1:].reshape(G, N), mask=mb[1:].reshape(G, W))
    b = S.sample_energy(xc, N, tc, log_weight=lb[1:].clone().reshape(G, N), mask=mb[1:].clone().reshape(G, W))
    assert same_bits(a.detach(), b.detach())
    ga, gb = torch.autograd.grad(a, (xu, tu), g), torch.autograd.grad(b, (xc, tc), g)
    assert same_bits(ga[0], gb[0]) and same_bits(ga[1], gb[1])
    wide, tw = torch.randn(G * N, 2 * W, generator=gen).to(DEV).requires_grad_(True), torch.randn(G, 2 * W, generator=gen).to(DEV).requires_grad_(True)
    lw2, m2 = torch.randn(G, 2 * N, generator=gen).to(DEV), (torch.rand(G, 2 * W, generator=gen) > 0.4).to(DEV)
    xs, ts, ls, ms = wide[:, ::2], tw[:, ::2], lw2[:, ::2], m2[:, ::2]                      # non-contiguous views, a bool mask
    xk, tk = xs.detach().clone().requires_grad_(True), ts.detach().clone().requires_grad_(True)
    assert not xs.is_contiguous() and not ls.is_contiguous()
    c1, c2 = S.sample_energy(xs, N, ts, log_weight=ls, mask=ms), S.sample_energy(xk, N, tk, log_weight=ls.clone(), mask=ms.clone())
    assert same_bits(c1.detach(), c2.detach())
    g1, g2 = torch.autograd.grad(c1, (wide, tw), g), torch.autograd.grad(c2, (xk, tk), g)
    assert same_bits(g1[0][:, ::2], g2[0]) and same_bits(g1[1][:, ::2], g2[1]) and float(g1[0][:, 1::2].abs().max()) == 0


@pytest.mark.parametrize('shape', E.SHAPES, ids=str)
def test_a_mask_of_ones_without_weights_gives_the_bits_of_the_unweighted_kernel(shape):
    G, N, V = shape
    c = _case(shape, None, True)
    x, y = np.where(c['obs'][:, None], c['x'], 0.25).astype(np.float32), np.where(c['obs'], c['y'], -1.5).astype(np.float32)      # (finite everywhere)
    for fair in (True, False):
        for mask in (torch.ones(G, V, device=DEV), 'nan'):
            xa, ya = _dev(x).reshape(G * N, V).requires_grad_(True), _dev(y).requires_grad_(True)
            xb, yb = _dev(x).reshape(G * N, V).requires_grad_(True), _dev(y).requires_grad_(True)
            a, b = S.sample_energy(xa, N, ya, fair=fair, mask=mask), S.sample_energy(xb, N, yb, fair=fair)
            assert type(a.grad_fn).__name__.startswith('_SampleEnergyWeighted') and not type(b.grad_fn).__name__.startswith('_SampleEnergyWeighted')
            assert same_bits(a.detach(), b.detach())
            ga, gb = torch.autograd.grad(a, (xa, ya), _dev(c['g'])), torch.autograd.grad(b, (xb, yb), _dev(c['g']))
            assert same_bits(ga[0], gb[0]) and same_bits(ga[1], gb[1])


@pytest.mark.parametrize('shape', E.SHAPES, ids=str)
def test_a_masked_call_gives_the_bits_of_the_unmasked_kernel_on_the_compacted_columns(shape):
    """Score by score: the unweighted kernel on the observed columns of that score alone (V changes, so do the chunk boundaries:
    the chain over v does not show them)."""
    G, N, V = shape
    c = _case(shape, None, True)
    for fair in (True, False):
        e, gx, gy = _run(c, fair)
        for i in range(G):
            o = c['obs'][i]
            if not o.any():
                assert float(e[i]) == 0 and float(gx[i].abs().max()) == 0 and float(gy[i].abs().max()) == 0
                continue
            xc, yc = E.compact(c['x'][i:i + 1], c['y'][i:i + 1], o)
            xd, yd = _dev(xc).reshape(N, -1).requires_grad_(True), _dev(yc).requires_grad_(True)
            ec = S.sample_energy(xd, N, yd, fair=fair)
            gxc, gyc = torch.autograd.grad(ec, (xd, yd), _dev(c['g'][i:i + 1]))
            od = _dev(o)
            assert same_bits(e[i:i + 1], ec.detach()), (i, fair)
            assert same_bits(gx[i][:, od], gxc) and same_bits(gy[i][od], gyc[0]), (i, fair)


@pytest.mark.parametrize('shape', E.SHAPES, ids=str)
def test_equal_weights_against_the_unweighted_kernel_within_the_sum_of_the_two_bounds(shape):
    G, N, V = shape
    c = _case(shape, None, True)
    x, y = np.where(c['obs'][:, None], c['x'], 0.25).astype(np.float32), np.where(c['obs'], c['y'], -1.5).astype(np.float32)
    logw = np.full((G, N), -2.75, np.float32)
    for fair in (True, False):
        rw, ru = E.energy(x, y, logw, None, fair, c['g']), E.energy(x, y, None, None, fair, c['g'])
        xa, ya = _dev(x).reshape(G * N, V).requires_grad_(True), _dev(y).requires_grad_(True)
        xb, yb = _dev(x).reshape(G * N, V).requires_grad_(True), _dev(y).requires_grad_(True)
        a, b = S.sample_energy(xa, N, ya, fair=fair, log_weight=_dev(logw)), S.sample_energy(xb, N, yb, fair=fair)
        ga, gb = torch.autograd.grad(a, (xa, ya), _dev(c['g'])), torch.autograd.grad(b, (xb, yb), _dev(c['g']))
        assert ((a - b).detach().abs().double().cpu().numpy() <= rw['E'] + ru['E']).all()
        assert ((ga[0] - gb[0]).abs().double().cpu().numpy().reshape(G, N, V) <= rw['E_x'] + ru['E_x']).all()
        assert ((ga[1] - gb[1]).abs().double().cpu().numpy() <= rw['E_y'] + ru['E_y']).all()


# ---- special values: checked with == where an exact zero is promised ------------------------------------------------------------------

def test_a_dead_sample_holding_nan_or_inf_is_the_set_without_it():
    """Sample 3 has a -Inf weight and holds NaN / Inf: the value and the other gradients are those of the call without it, within the
    sum of the two bounds (N differs: another tile layout); its own gradient row is an exact zero."""
    G, N, V = 2, 41, 19
    c = E.make_case((G, N, V), 1.0)
    logw, x = c['logw'].copy(), c['x'].copy()
    logw[:, 3] = -INF
    x[0, 3], x[1, 3] = NAN, INF
    keep = [n for n in range(N) if n != 3]
    for fair in (True, False):
        ea, gxa, gya = _run(dict(c, x=x, logw=logw), fair)
        eb, gxb, gyb = _run(dict(c, x=np.ascontiguousarray(x[:, keep]), logw=np.ascontiguousarray(logw[:, keep])), fair)
        r, full = E.energy(x[:, keep], c['y'], logw[:, keep], None, fair, c['g']), E.energy(x, c['y'], logw, None, fair, c['g'])
        assert bool(torch.isfinite(ea).all()) and bool((gxa[:, 3] == 0).all())
        assert ((ea - eb).abs().double().cpu().numpy() <= r['E'] + full['E']).all()
        assert ((gxa[:, keep] - gxb).abs().double().cpu().numpy() <= r['E_x'] + full['E_x'][:, keep]).all()
        assert ((gya - gyb).abs().double().cpu().numpy() <= r['E_y'] + full['E_y']).all()
        assert E.ratio(ea.cpu().numpy(), full['energy'], full['E']) <= 1.0 and E.ratio(gxa.cpu().numpy(), full['grad_x'], full['E_x']) <= 1.0


@pytest.mark.parametrize('bad', [[-INF] * 5, [0.0, NAN, 0.0, 0.0, 0.0], [0.0, INF, 0.0, 0.0, 0.0]], ids=['all-inf', 'nan', '+inf'])
def test_an_unusable_weight_row_is_nan_and_its_neighbours_keep_their_bits(bad):
    G, N, V = 3, 5, 18
    c = E.make_case((G, N, V), 1.0, masked=True)
    for i in range(G):
        E.set_observed(c, i, 0, True)      # (every group has an observed column and a gap)
        E.set_observed(c, i, 1, False)
    clean = _run(c, True)
    logw = c['logw'].copy()
    logw[1] = bad
    e, gx, gy = _run(dict(c, logw=logw), True)
    assert bool(torch.isnan(e[1])) and same_bits(e[[0, 2]], clean[0][[0, 2]])
    assert same_bits(gx[[0, 2]], clean[1][[0, 2]]) and same_bits(gy[[0, 2]], clean[2][[0, 2]])
    obs = _dev(c['obs'][1])
    assert bool(torch.isnan(gy[1][obs]).all()) and bool((gy[1][~obs] == 0).all())
    assert bool(torch.isnan(gx[1][:, obs]).all()) and bool((gx[1][:, ~obs] == 0).all())


def test_one_live_sample_under_fair_is_nan_and_its_unfair_score_is_its_distance():
    x, y = torch.tensor([[3.0, 4.0], [NAN, 1.0], [INF, -INF]], device=DEV, requires_grad=True), torch.zeros(1, 2, device=DEV)
    lw = torch.tensor([[0.0, -INF, -INF]], device=DEV)
    e = S.sample_energy(x, 3, y, log_weight=lw)
    gx, = torch.autograd.grad(e.sum(), x)
    assert bool(torch.isnan(e).all()) and bool(torch.isnan(gx[0]).all()) and bool((gx[1:] == 0).all())
    e0 = S.sample_energy(x, 3, y, fair=False, log_weight=lw)
    g0, = torch.autograd.grad(e0.sum(), x)
    assert e0.item() == 5.0 and bool((g0[1:] == 0).all()) and torch.allclose(g0[0], torch.tensor([0.6, 0.8], device=DEV), rtol=1e-6, atol=0)


def test_a_fully_masked_score_is_zero_and_nothing_under_the_mask_reaches_anything():
    G, N, V = 3, 6, 21
    c = E.make_case((G, N, V), 4.0, masked=True)
    c['obs'][1] = False
    c['x'][1], c['y'][1] = NAN, INF
    c['g'][2] = INF                                       # (gaps get zeros by selection, whatever g is)
    E.set_observed(c, 2, 0, False)
    E.set_observed(c, 2, 1, True)
    E.set_observed(c, 0, 1, True)
    gap = _dev(~c['obs'])
    for fair in (True, False):
        e, gx, gy = _run(c, fair)
        assert float(e[1]) == 0 and bool((gx[1] == 0).all()) and bool((gy[1] == 0).all())
        assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(gx[0]).all()) and bool(torch.isfinite(gy[0]).all())
        assert bool((gy[gap] == 0).all()) and bool((gx[gap[:, None].expand_as(gx)] == 0).all())
        c2 = dict(c, x=np.where(c['obs'][:, None], c['x'], 7.0).astype(np.float32), y=np.where(c['obs'], c['y'], -3.0).astype(np.float32))
        e2, gx2, gy2 = _run(c2, fair)      # the values under the mask do not matter, bit for bit
        assert same_bits(e, e2) and same_bits(gx[:2], gx2[:2]) and same_bits(gy[:2], gy2[:2])
        # engine.sample_energy_weighted_backward: the same launch without autograd
        hx, hy = engine.sample_energy_weighted_backward(_dev(c['g']), _dev(c['x']).reshape(G * N, V), _dev(c['y']), N, _dev(c['logw']),
                                                        _dev(c['obs']).float(), fair)
        assert same_bits(hx.reshape(G, N, V), gx) and same_bits(hy, gy)


def test_more_than_256_pooled_samples_take_the_tensor_op_route():
    G, N, W = 2, 257, 3
    c = E.make_case((G, N, W), 1.0, masked=True)
    xd = _dev(c['x']).reshape(G * N, W).requires_grad_(True)
    e = S.sample_energy(xd, N, _dev(c['y']), log_weight=_dev(c['logw']), mask=_dev(c['obs']))
    assert e.grad_fn is not None and not type(e.grad_fn).__name__.startswith('_SampleEnergy')
    r = E.energy(c['x'], c['y'], c['logw'], c['obs'], True)
    assert E.ratio(e.detach().cpu().numpy(), r['energy'], r['E']) <= 1.0
    gx, = torch.autograd.grad(e.sum(), xd)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0


# ---- the buffer contract: every output element written, no byte outside (tests/buffer_arena.py) --------------------------------

def _hold(call, what):
    assert call.rc == 0, (what, call.name, call.rc)
    fn = getattr(_lib.lib(), call.name)
    got = {}
    for offset in (0, 1):
        for fill in FILLS:
            tag = f'{what} {call.name} fill {fill:#04x} offset {offset}'
            sizes = [t.numel() * t.element_size() for t in call.tensors.values()]
            arena = Arena(DEV, fill, sum(Arena.room(n) for n in sizes) + (1 << 16))
            placed = place(call, arena, offset)
            rc = replay(fn, call, placed)
            torch.cuda.current_stream().synchronize()
            assert rc == 0, (tag, rc)
            arena.check(tag)
            for p in placed.values():
                if not p.is_output:
                    assert same_bits(p.view, p.original.reshape(-1)), f'{tag}: an input was changed'
            got[offset, fill] = {ptr: p.view.clone() for ptr, p in placed.items() if p.is_output}
            assert got[offset, fill], f'{tag}: the recording names no output'
    for key, outs in got.items():      # the engine's own bits whatever the memory held and wherever it sat
        for ptr, out in outs.items():
            assert same_bits(out, call.tensors[ptr].reshape(-1)), f'{what} {call.name} {key}: differs from the engine\'s result'


@pytest.mark.parametrize('optional', [True, False], ids=['all outputs, weights and mask', 'required only, mask by NaN'])
@pytest.mark.parametrize('shape', [(3, 5, 3), (2, 65, 130)], ids=str)
def test_buffer_contract_of_the_two_entry_points(shape, optional):
    G, N, V = shape
    c = _case(shape, 1.0, True)
    ys, y, g = _dev(c['x']).reshape(G * N, V), _dev(c['y']), _dev(c['g'])
    lw, mk = (_dev(c['logw']), _dev(c['obs']).float()) if optional else (None, 'nan')

    def thunk():
        engine.sample_energy(ys, N, y, fair=optional, log_weight=lw, mask=mk)
        engine.sample_energy_weighted_backward(g, ys, y, N, lw, mk, fair=optional, grad_target=optional)
    with recorded_calls(engine) as rec:
        thunk()
    torch.cuda.current_stream().synchronize()
    _hold(rec.named('snsde_sample_energy_weighted'), f'{shape}')
    _hold(rec.named('snsde_sample_energy_weighted_backward'), f'{shape}')


def test_forward_and_backward_replay_from_one_graph_on_new_values():
    G, N, W = 7, 12, 50
    gen = torch.Generator().manual_seed(6)

    def draw():
        return [torch.randn(G * N, W, generator=gen).to(DEV), torch.randn(G, W, generator=gen).to(DEV), torch.randn(G, generator=gen).to(DEV),
                (3 * torch.randn(G, N, generator=gen)).to(DEV), (torch.rand(G, W, generator=gen) > 0.4).float().to(DEV)]
    first, second = draw(), draw()
    second[0][1] = second[0][0]
    sx, sy, sg, sl, sm = (t.clone() for t in first)
    sx.requires_grad_(True)
    sy.requires_grad_(True)

    def step(x, y, g, lw, mk):
        e = S.sample_energy(x, N, y, log_weight=lw, mask=mk)
        gx, gy = torch.autograd.grad(e, (x, y), g)
        return e.detach(), gx, gy

    side = torch.cuda.Stream()      # (warm-up outside the capture, on a side stream as capture asks)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sy, sg, sl, sm)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(sx, sy, sg, sl, sm)
    with torch.no_grad():
        for dst, src in zip((sx, sy, sg, sl, sm), second):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = step(second[0].clone().requires_grad_(True), second[1].clone().requires_grad_(True), *second[2:])
    for name, a, b in zip(('energy', 'grad_ys', 'grad_target'), static, eager):
        assert same_bits(a, b), name
    assert float(static[0].abs().max()) > 0 and float(static[1].abs().max()) > 0


# ---- the filtering recipe ------------------------------------------------------------------------------------------------------------------

TS = torch.tensor([0.0, 0.75, 2.25, 4.0])
CASE = STEP_OFFSET_CASES[1]      # 'lean general': B = 8 input rows, H = 32


def _module():
    c = CASE
    pr = make_problem(9, c.io, c.no, c.NL, c.B, c.H, c.C, 7)
    m = S.Diffusion_model(c.C, c.H, c.H, c.NL, input_option=c.io, noise_option=c.no)
    with torch.no_grad():
        for name, q in m.named_parameters():
            q.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(DEV).requires_grad_(False)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    return m, torch.from_numpy(pr['y0']).to(DEV)


def _likelihood(Sn):
    def fn(k, yk):      # a Gaussian observation of three state components, fused
        obs = torch.full((yk.shape[0] // Sn, 3), 0.1 * k, device=yk.device)
        return engine.sample_loglik(yk[:, :3].contiguous(), Sn, obs, std=0.5, stats=True)[1]
    return fn


def test_the_filtering_recipe_on_sdeint_filter_against_float64():
    """8 rows x 8 particles, 3 observations, resampling where the effective sample size falls under half: between two resamplings the
    weights are not uniform.  sample_energy(filter_particles(r.ys, r.ancestor, S), S, target, log_weight=r.log_weight) against the
    float64 statement on the gathered particles, with a target that has gaps."""
    assert CASE.B == 8
    m, y0 = _module()
    Sn, B, H = 8, CASE.B, CASE.H
    r = S.sdeint_filter(m, y0, TS.to(DEV), _likelihood(Sn), method='euler', dt=0.25, options={'samples': Sn, 'seed': 77}, threshold=0.5,
                        generator=torch.Generator(DEV).manual_seed(5))
    T = r.ys.shape[0]
    assert tuple(r.log_weight.shape) == (T, B, Sn) and float((r.log_weight - r.log_weight[..., :1]).abs().max()) > 0
    target = torch.randn(T, B, H, generator=torch.Generator().manual_seed(6))
    target[2, :, ::3] = NAN
    parts = S.filter_particles(r.ys, r.ancestor, Sn)
    for fair in (True, False):
        e = S.sample_energy(parts, Sn, target.to(DEV), fair=fair, log_weight=r.log_weight, mask='nan')
        ref = E.energy(parts.reshape(T * B, Sn, H).cpu().numpy(), target.reshape(T * B, H).numpy(), r.log_weight.reshape(T * B, Sn).cpu().numpy(),
                       ~torch.isnan(target).reshape(T * B, H).numpy(), fair)
        ratio = E.ratio(e.reshape(-1).cpu().numpy(), ref['energy'], ref['E'])
        print(f'filter recipe fair={fair}: err / bound {ratio:.3f}')
        assert tuple(e.shape) == (T, B) and ratio <= 1.0
