"""snsde_sample_crps / snsde_sample_quantiles and their adjoints on the GPU, through sample_crps / sample_quantiles / crps_loss.

Shapes (groups, N, W): (1, 2, 1) - the smallest fair score, one live lane, two of the four waves without a sample; (3, 5, 33) - odd
sizes, a quarter split that is not even; (2, 64, 130) - three column tiles, the last with two live lanes; (1, 256, 4) - the LDS cap;
(9000, 3, 2) - more tiles than the block cap (8192): the grid stride.  u = 2^-24 throughout.  The float64 references are computed
once per shape from the float32 inputs and shared."""
import copy
import functools

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine, train
from tests.helpers import make_problem
from tests.score_special_cases import SCORE_SHAPES

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

SHAPES = SCORE_SHAPES
U = 2.0 ** -24
QS = (0.0, 0.1, 0.5, 0.9, 1.0)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs with planted ties - in every (group, column) sample 1 duplicates sample 0 and, where N > 2, the observation equals
    sample 2 - and everything the float64 formulas give for them.  Never modified."""
    G, N, W = shape
    rng = np.random.default_rng(G + N + W)
    x = (2.0 * rng.standard_normal((G, N, W)) + 0.5).astype(np.float32)
    x[:, 1] = x[:, 0]
    y = rng.standard_normal((G, W)).astype(np.float32)
    if N > 2:
        y[:] = x[:, 2]
    g = rng.standard_normal((G, W)).astype(np.float32)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = x64 - y64[:, None]
    order = np.sort(x64, axis=1)
    c = np.empty_like(x64)      # strict counts from a sort of each column (no (N, N) array at G = 9000)
    for gi in range(G):
        for w in range(W):
            col = order[gi, :, w]
            c[gi, :, w] = np.searchsorted(col, x64[gi, :, w], 'left') - (N - np.searchsorted(col, x64[gi, :, w], 'right'))
    out = dict(x=x, y=y, g=g, d=d, c=c, rank=(d < 0).sum(1), ties=(d == 0).sum(1), sign=np.sign(d))
    for fair in (True, False):
        D = N - 1 if fair else N
        out[fair] = dict(crps=np.abs(d).sum(1) / N - (c * d).sum(1) / (N * D),
                         scale=np.abs(d).sum(1) / N + (np.abs(c) * np.abs(d)).sum(1) / (N * D),      # A + B'
                         gx=g.astype(np.float64)[:, None] * (np.sign(d) / N - c / (N * D)),
                         gx_scale=np.abs(g.astype(np.float64))[:, None] * (1.0 / N + np.abs(c) / (N * D)),
                         gy=-g.astype(np.float64) * np.sign(d).sum(1) / N)
    # permutation ranks, ties by index: a stable argsort
    perm = np.argsort(x64, axis=1, kind='stable')
    out['perm'] = perm
    out['sorted'] = np.take_along_axis(x64, perm, axis=1)
    return out


def _dev(a):
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize('fair', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_crps_rank_and_ties_against_float64(shape, fair):
    """|err| <= (2 N + 4) u (A + B'), A = sum |d_n| / N, B' = sum |c_n| |d_n| / (N D) in float64: d_n carries one rounding; the
    first sum adds N such non-negative terms (quarter by quarter, the four quarter sums then in order: no addition is deeper than
    N levels), the second adds N terms c_n d_n by fma (c_n an exact integer: one rounding per step on top of d_n's); one division
    each and the final subtraction.  rank and ties are integer counts: exact."""
    G, N, W = shape
    c = _case(shape)
    xd, yd = _dev(c['x']).reshape(G * N, W), _dev(c['y'])
    crps, rank, ties = S.sample_crps(xd, N, yd, fair=fair, rank=True)
    again = S.sample_crps(xd, N, yd, fair=fair, rank=True)
    assert tuple(crps.shape) == (G, W) and crps.dtype == rank.dtype == ties.dtype == torch.float32
    err = np.abs(crps.double().cpu().numpy() - c[fair]['crps'])
    bound = (2 * N + 4) * U * c[fair]['scale']
    print(f'sample_crps {shape} fair={fair}: err / bound max {np.max(err / bound):.3f}')
    assert (err <= bound).all()
    assert np.array_equal(rank.cpu().numpy(), c['rank'].astype(np.float32)) and np.array_equal(ties.cpu().numpy(), c['ties'].astype(np.float32))
    assert all(torch.equal(a, b) for a, b in zip((crps, rank, ties), again))              # the same bits on every launch
    assert torch.equal(S.sample_crps(xd, N, yd, fair=fair), crps)                         # rank = ties = NULL
    if N > 2:
        assert int(c['ties'].min()) >= 1


@pytest.mark.parametrize('fair', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_crps_gradients_against_the_float64_formula_with_planted_ties(shape, fair):
    """grad_ys = g (sign(d_n) / N - c_n / (N D)): two divisions, one subtraction and one product, each one rounding: within
    4 u |g| (1 / N + |c_n| / (N D)).  grad_target = -(g sum sign(d_n)) / N: an exact integer sum, a product and a division: within
    (N + 2) u |g|.  Exact zeros where the formula is zero (a sample equal to the observation whose count is zero)."""
    G, N, W = shape
    c = _case(shape)
    xd, yd = _dev(c['x']).reshape(G * N, W).requires_grad_(True), _dev(c['y']).requires_grad_(True)
    crps = S.sample_crps(xd, N, yd, fair=fair)
    assert type(crps.grad_fn).__name__.startswith('_SampleCRPS')
    gx, gy = torch.autograd.grad(crps, (xd, yd), _dev(c['g']))
    gx2, gy2 = torch.autograd.grad(S.sample_crps(xd, N, yd, fair=fair), (xd, yd), _dev(c['g']))
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2)
    r = c[fair]
    gxn, gyn = gx.double().cpu().numpy().reshape(G, N, W), gy.double().cpu().numpy()
    ex, ey = np.abs(gxn - r['gx']), np.abs(gyn - r['gy'])
    print(f'sample_crps backward {shape} fair={fair}: grad_ys err / bound max {np.max(ex / (4 * U * r["gx_scale"])):.3f}, '
          f'grad_target err max {np.max(ey / ((N + 2) * U * np.abs(c["g"]))):.3f} of the bound')
    assert (ex <= 4 * U * r['gx_scale']).all()
    assert (ey <= (N + 2) * U * np.abs(c['g'].astype(np.float64))).all()
    zero = r['gx'] == 0
    assert (gxn[zero] == 0).all()
    # only ys requires grad: grad_target = NULL
    x2 = xd.detach().requires_grad_(True)
    assert torch.equal(torch.autograd.grad(S.sample_crps(x2, N, yd.detach(), fair=fair), x2, _dev(c['g']))[0], gx)
    y2 = yd.detach().requires_grad_(True)
    assert torch.equal(torch.autograd.grad(S.sample_crps(xd.detach(), N, y2, fair=fair), y2, _dev(c['g']))[0], gy)


@pytest.mark.parametrize('shape', SHAPES)
def test_quantiles_and_their_backward(shape):
    """value = fma(frac, x_(k+1) - x_(k), x_(k)): the difference and the fma round once each, on float32 order statistics that
    are exact: within 3 u (|x_(k)| + |x_(k+1)|) of the float64 value from the same k, frac.  q = 0 and q = 1 are min and max."""
    G, N, W = shape
    c = _case(shape)
    xd = _dev(c['x']).reshape(G * N, W).requires_grad_(True)
    ks, fracs = engine.quantile_positions(QS, N)
    out = S.sample_quantiles(xd, N, QS)
    assert tuple(out.shape) == (len(QS), G, W) and type(out.grad_fn).__name__.startswith('_SampleQuantiles')
    assert torch.equal(out, S.sample_quantiles(xd.detach(), N, QS))
    srt = c['sorted']
    for i, (k, f) in enumerate(zip(ks, fracs)):
        lo, hi = srt[:, k], srt[:, min(k + 1, N - 1)]
        want = lo if f == 0.0 else lo + f * (hi - lo)
        assert (np.abs(out[i].detach().double().cpu().numpy() - want) <= 3 * U * (np.abs(lo) + np.abs(hi))).all(), (i, k, f)
    x3 = xd.detach().reshape(G, N, W)
    assert torch.equal(out[0].detach(), x3.min(1).values) and torch.equal(out[-1].detach(), x3.max(1).values)
    # backward, one level at a time: g (1 - frac) to rank k, g frac to rank k + 1 (one non-zero where frac == 0), zeros elsewhere
    g = _dev(c['g'])
    perm = c['perm']
    for i, (k, f) in enumerate(zip(ks, fracs)):
        gx, = torch.autograd.grad(S.sample_quantiles(xd, N, [QS[i]])[0], xd, g)
        gxn = gx.cpu().numpy().reshape(G, N, W)
        want = np.zeros((G, N, W), np.float32)
        np.put_along_axis(want, perm[:, k:k + 1], (c['g'] * (np.float32(1) - np.float32(f)))[:, None], axis=1)
        if f != 0.0:
            np.put_along_axis(want, perm[:, k + 1:k + 2], (c['g'] * np.float32(f))[:, None], axis=1)
        assert np.array_equal(gxn, want), (i, k, f)
        assert ((gxn != 0).sum(1) == (1 if f == 0.0 else 2)).all()
        assert (np.abs(gxn.astype(np.float64).sum(1) - c['g']) <= 2 * U * np.abs(c['g'])).all()
    # the planted duplicate (samples 0 and 1): the lower index holds the lower rank
    r0 = np.argsort(perm, axis=1)      # rank of each sample
    assert (r0[:, 1] == r0[:, 0] + 1).all()
    # all levels in one launch: the sum of the single-level gradients, q ascending
    gall, = torch.autograd.grad(S.sample_quantiles(xd, N, QS), xd, g.expand(len(QS), G, W).contiguous())
    assert bool(torch.isfinite(gall).all()) and int((gall != 0).sum()) <= 2 * len(QS) * G * W


def test_pooled_ensemble_layout_equals_the_permuted_single_member_call():
    O, M, G, Sn, W = 2, 3, 5, 4, 70
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(O, M, G * Sn, W, generator=gen)
    x[:, 1, 3] = x[:, 0, 2]      # ties across members
    y, g = torch.randn(O, G, W, generator=gen), torch.randn(O, G, W, generator=gen)
    flat = x.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W).contiguous()
    xa, xb, ya, yb = (t.to(DEV).requires_grad_(True) for t in (x, flat, y, y))
    a = S.sample_crps(xa, Sn, ya, members=M, rank=True)
    b = S.sample_crps(xb, M * Sn, yb, rank=True)
    assert tuple(a[0].shape) == (O, G, W) and all(torch.equal(u, v) for u, v in zip(a, b))
    ga, gb = torch.autograd.grad(a[0], (xa, ya), g.to(DEV)), torch.autograd.grad(b[0], (xb, yb), g.to(DEV))
    assert torch.equal(ga[0].reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), gb[0]) and torch.equal(ga[1], gb[1])
    qa, qb = S.sample_quantiles(xa, Sn, QS, members=M), S.sample_quantiles(xb, M * Sn, QS)
    assert torch.equal(qa, qb)
    gq = torch.randn(len(QS), O, G, W, generator=gen).to(DEV)
    ha, hb = torch.autograd.grad(qa, xa, gq)[0], torch.autograd.grad(qb, xb, gq)[0]
    assert torch.equal(ha.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), hb)
    # against float64 of the pooled set
    ref = S.sample_crps(flat.double(), M * Sn, y.double())
    assert float((a[0].detach().double().cpu() - ref).abs().max()) <= (2 * M * Sn + 4) * U * 8


def test_unaligned_and_non_contiguous_inputs_give_the_bits_of_their_clones():
    G, N, W = 4, 6, 64
    buf = torch.randn(G * N * W + 1, device=DEV)
    tb = torch.randn(G * W + 1, device=DEV)
    a = S.sample_crps(buf[1:].reshape(G * N, W), N, tb[1:].reshape(G, W), rank=True)      # 4 bytes off a 16-byte boundary
    b = S.sample_crps(buf[1:].clone().reshape(G * N, W), N, tb[1:].clone().reshape(G, W), rank=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(S.sample_quantiles(buf[1:].reshape(G * N, W), N, QS), S.sample_quantiles(buf[1:].clone().reshape(G * N, W), N, QS))
    wide = torch.randn(G * N, 2 * W, device=DEV).requires_grad_(True)
    tw = torch.randn(G, 2 * W, device=DEV).requires_grad_(True)
    xs, ts = wide[:, ::2], tw[:, ::2]                                                     # non-contiguous views
    xc, tc = xs.detach().clone().requires_grad_(True), ts.detach().clone().requires_grad_(True)
    assert not xs.is_contiguous()
    c1, c2 = S.sample_crps(xs, N, ts), S.sample_crps(xc, N, tc)
    assert torch.equal(c1, c2)
    g = torch.randn(G, W, device=DEV)
    g1, g2 = torch.autograd.grad(c1, (wide, tw), g), torch.autograd.grad(c2, (xc, tc), g)
    assert torch.equal(g1[0][:, ::2], g2[0]) and torch.equal(g1[1][:, ::2], g2[1]) and float(g1[0][:, 1::2].abs().max()) == 0
    assert torch.equal(S.sample_quantiles(xs, N, QS), S.sample_quantiles(xc, N, QS))


def test_more_than_256_pooled_samples_take_the_tensor_op_route():
    G, N, W = 2, 257, 3
    gen = torch.Generator().manual_seed(5)
    x, y = torch.randn(G * N, W, generator=gen), torch.randn(G, W, generator=gen)
    xd = x.to(DEV).requires_grad_(True)
    crps = S.sample_crps(xd, N, y.to(DEV))
    assert not type(crps.grad_fn).__name__.startswith('_SampleCRPS')
    ref = S.sample_crps(x.double(), N, y.double())
    assert float((crps.detach().double().cpu() - ref).abs().max()) <= (2 * N + 4) * U * 8
    q = S.sample_quantiles(xd, N, QS)
    qref = torch.quantile(x.double().reshape(G, N, W), torch.tensor(QS, dtype=torch.float64), dim=1)
    assert float((q.detach().double().cpu() - qref).abs().max()) <= 3 * U * 2 * float(x.abs().max())
    # nine levels at N within the cap: tensor ops as well
    nine = S.sample_quantiles(xd[:2 * 8], 8, [i / 8 for i in range(9)])
    assert not type(nine.grad_fn).__name__.startswith('_SampleQuantiles') and tuple(nine.shape) == (9, 2, W)


def test_forward_and_backward_replay_from_one_graph_on_new_values():
    G, N, W = 7, 12, 100
    gen = torch.Generator().manual_seed(6)
    first = [torch.randn(G * N, W, generator=gen).to(DEV), torch.randn(G, W, generator=gen).to(DEV), torch.randn(G, W, generator=gen).to(DEV)]
    second = [torch.randn(G * N, W, generator=gen).to(DEV), torch.randn(G, W, generator=gen).to(DEV), torch.randn(G, W, generator=gen).to(DEV)]
    second[0][1] = second[0][0]
    sx, sy, sg = (t.clone() for t in first)
    sx.requires_grad_(True)
    sy.requires_grad_(True)

    def step(x, y, g):
        crps, rank, ties = S.sample_crps(x, N, y, rank=True)
        q = S.sample_quantiles(x, N, QS)
        gx, gy = torch.autograd.grad([crps, q], (x, y), [g, g.expand(len(QS), G, W).contiguous()])
        return crps.detach(), rank, ties, q.detach(), gx, gy

    side = torch.cuda.Stream()      # (warm-up outside the capture, on a side stream as capture asks)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sy, sg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(sx, sy, sg)
    with torch.no_grad():
        for dst, src in zip((sx, sy, sg), second):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = step(second[0].clone().requires_grad_(True), second[1].clone().requires_grad_(True), second[2])
    for name, a, b in zip(('crps', 'rank', 'ties', 'quantiles', 'grad_ys', 'grad_target'), static, eager):
        assert torch.equal(a, b), name
    assert float(static[0].abs().max()) > 0 and float(static[4].abs().max()) > 0


TIMES = np.array([0., 1., 2., 3., 4., 5.], np.float32)


def _solve_and_score(pr, target, B, Sn, H):
    m = S.Diffusion_model(3, H, H, 2, input_option=4, noise_option=17)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(DEV)
    coeffs = torch.from_numpy(pr['coeffs']).to(DEV).requires_grad_(True)
    m.set_X(coeffs, torch.from_numpy(TIMES).to(DEV))
    y0 = torch.from_numpy(pr['y0']).to(DEV).repeat_interleave(Sn, 0).requires_grad_(True)
    ys = S.sdeint(m, y0, torch.tensor([0., 5.], device=DEV), method='euler', dt=1.0, options={'samples': Sn, 'sample_grad': True, 'seed': 17})
    assert tuple(ys.shape) == (2, B * Sn, H)
    ys.retain_grad()
    crps = S.sample_crps(ys[-1], Sn, target)
    crps.mean().backward()
    return m, coeffs, y0, ys, crps


def test_a_sampled_solve_trains_through_the_score():
    B, Sn, H = 5, 4, 64
    pr = make_problem(23, 4, 17, 2, B, H, 3, len(TIMES), times=TIMES)
    target = torch.from_numpy(np.random.default_rng(2).standard_normal((B, H)).astype(np.float32)).to(DEV)
    m, coeffs, y0, ys, crps = _solve_and_score(pr, target, B, Sn, H)
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads.update(y0=y0.grad, coeffs=coeffs.grad)
    for n, gr in grads.items():
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, n
    m2, coeffs2, y02, ys2, crps2 = _solve_and_score(pr, target, B, Sn, H)
    assert torch.equal(crps, crps2) and torch.equal(y0.grad, y02.grad) and torch.equal(coeffs.grad, coeffs2.grad)
    for (n, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p.grad, p2.grad), n
    # dL/d ys of the mean score against the float64 formula: g = 1 / (B H)
    x64 = ys.detach()[-1].double().cpu().numpy().reshape(B, Sn, H)
    d = x64 - target.double().cpu().numpy()[:, None]
    c = (x64[:, None, :, :] < x64[:, :, None, :]).sum(2) - (x64[:, None, :, :] > x64[:, :, None, :]).sum(2)
    g = 1.0 / (B * H)
    want = g * (np.sign(d) / Sn - c / (Sn * (Sn - 1)))
    got = ys.grad[-1].double().cpu().numpy().reshape(B, Sn, H)
    assert (np.abs(got - want) <= 4 * U * g * (1.0 / Sn + np.abs(c) / (Sn * (Sn - 1))) + U * np.abs(want)).all()      # (+ u: g = 1 / 320 itself is rounded)
    assert float(ys.grad[0].abs().max()) == 0


def test_ensemble_trains_on_crps_loss_through_a_graphed_step():
    M, Sn, B, H, Cn, out_time = 2, 2, 4, 64, 3, 2
    pr = make_problem(31, 4, 17, 2, B, H, Cn, len(TIMES), times=TIMES)
    models = []
    for mi in range(M):
        torch.manual_seed(700 + mi)
        func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=17)
        models.append(S.NeuralSDE_forecasting(func, Cn, out_time, H, Cn).to(DEV))
    ens = S.Ensemble(models).train()
    ens2 = copy.deepcopy(ens)
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    true = torch.from_numpy(np.random.default_rng(4).standard_normal((B, out_time, Cn)).astype(np.float32)).to(DEV)
    lengths = torch.full((B,), len(TIMES) - 1, device=DEV)
    kwargs = {'method': 'euler', 'options': {'seed': 9, 'samples': Sn, 'ensemble_samples': True, 'ensemble_grad': True, 'sample_grad': True}}
    base = S.crps_loss(Sn, members=M)
    seen = []

    def loss_fn(pred, y):
        assert tuple(pred.shape) == (M, B * Sn, out_time, Cn)
        loss = base(pred, y)
        seen.append(loss.detach())      # (under capture: a view of the recording's loss, refreshed by every replay)
        return loss

    opt = torch.optim.Adam(ens.parameters(), lr=1e-3, capturable=True)
    for _ in range(2):
        loss_fn(ens(times, (coeffs,), lengths, **kwargs), true).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    eager = [t.clone() for t in seen]
    del seen[:]
    opt2 = torch.optim.Adam(ens2.parameters(), lr=1e-3, capturable=True)
    graphed = train.GraphedStep(ens2, times, opt2, loss_fn, kwargs, torch.device(DEV), warmup=1)
    graphed((coeffs,), true, lengths)      # the warm-up step of this batch shape: eager
    graphed((coeffs,), true, lengths)      # recorded, then replayed
    torch.cuda.synchronize()
    assert graphed.disabled is None and graphed.replays == 1, graphed.disabled
    assert len(seen) == 2 and torch.equal(seen[0], eager[0]) and torch.equal(seen[1], eager[1])
    assert float(eager[1]) > 0 and not torch.equal(eager[0], eager[1])
    for p, p2 in zip(ens.parameters(), ens2.parameters()):
        assert torch.equal(p, p2)
