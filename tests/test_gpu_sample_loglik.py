"""snsde_sample_loglik and its adjoint on the GPU, through sample_loglik / iwae_loss.

Shapes (groups G, pooled samples N, outer, width W), V = outer W.  The kernel's buckets follow from N alone: L = min(32, largest
power of two <= 256 / N) lanes per sample, chunks of CW = 64 L columns, RS = max(1, 4 / L) row parts per staged column; the
backward takes tiles of 256 columns.  (1, 1, 1, 1) - the smallest case; (3, 5, 2, 3) - odd sizes and the outer stride, fractional
weights; (2, 8, 1, 64) | (2, 8, 1, 65) - a 64-column boundary and one live tail column; (2, 7, 3, 130) - V = 390 from three
outer slices; (1, 256, 1, 4) - the cap of N (L = 1, RS = 4); (9000, 2, 1, 2) - more groups than the 8192-block cap; N on either
side of every edge of L - 8 | 9, 16 | 17, 32 | 33, 64 | 65 (RS 1 | 2), 128 | 129 (RS 2 | 4) - each with V at or one past its own
chunk width: (2, 8, 1, 2048), (1, 2, 1, 2049), (1, 9, 1, 1025), (2, 16, 2, 40), (2, 17, 1, 70), (2, 32, 1, 513), (2, 33, 1, 257),
(2, 64, 1, 256), (2, 65, 1, 129), (1, 128, 1, 128), (1, 129, 1, 65).
Where G >= 2, group 0 is fully masked and group 1 fully observed; the other masks drop about 40 % of the entries.  target AND ys
hold NaN at every masked-out position.  The float64 references are computed once per shape from the float32 inputs (and the
float32 logvar and inv_var the kernel receives) and shared.

The bounds, u = 2^-24, from the summation order include/snsde.h documents.  Dd = ceil(V / L) + log2 L is the depth of a
sub-lane's chain plus the butterfly.
  logpx: d = y - x rounds once (d^2: 2 u), m d once, the fmaf chain Dd times: q_n within (Dd + 3) u; count within Dd u; K =
  (float)log 2 pi + logvar is off by u log 2 pi + u |K|, K count rounds once, the closing fmaf once: with A_n = (|K| count +
  inv_var q_n) / 2, |err| <= (Dd + 6) u A_n + u (log 2 pi + |logvar|) count (second-order terms inside the slack); under norm
  the division adds (Dd + 2) u A_n, all over count.
  bound: a_n = logpx_n + logw_n rounds once: E_n = E_logpx,n + u |a_n|; logsumexp is 1-Lipschitz in max_n E_n.  Separately, its
  own arithmetic: a_n - max rounds within u |a_n - max| and expf / logf are within 2 ulp (4 u), so a term is off by
  (|a_n - max| + 4) u relatively and the weighted mean of |a_n - max| is at most the entropy, log N; the chain and butterfly of
  the sum ceil(N / 64) + 6; logf(sum) 4 u log N, logf(N) 4 u log N, the two additions 2 u (|max| + 2 log N):
  E_lse = u (2 |max_n a_n| + 11 log N + ceil(N / 64) + 16).
  sqerr: s_v adds N once-rounded residuals: (N + 1) u N abar_v, abar_v = mean_n |d_nv|; e_v = s_v / N one more u; e^2 doubles;
  m e once; the chain, butterfly and waves Dc = ceil(V / min(CW, 256)) + 9:
  |err| <= u ((2 N + 4) sum_v m_v |e_v| abar_v + (Dc + 4) sum_v m_v e_v^2).
  backward: p_n is formed from the float32 logpx: E'_n = E_logpx,n + u |a_n| + u |a_n - max|, p_n relatively within
  R = expm1(2 max_n E'_n) + 16 u (expf, the <= 9-deep block sum, the division).  grad_ys = ((c_n inv_var) m_v) d_nv, c_n =
  (gl_n + gb p_n) / count: |err| <= (|gb| p_n R + (|gl_n| + |gb| p_n) (Dd + 10) u) inv_var / count m_v |d_nv|; grad_target adds
  these over n plus N u sum_n |grad_ys|; grad_logw = gb p_n within |gb| p_n (R + 2 u).  float32 has no p_n below 2^-126: expf(a_n -
  max) of a path more than 87 below the best one flushes to zero (at V = 2048 the paths of a group lie hundreds apart), so p_n
  carries the absolute term TINY = 2^-126 beside p_n R, and each product that may underflow one more TINY.
The tensor-op statement in float32 (the routing tests): a term rounds at most 8 times and torch's sums are no deeper than V:
(V + 10) u A_n + u (log 2 pi + |logvar|) count, and E_lse with N in place of ceil(N / 64)."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine, train
from tests.helpers import make_problem
from tests.score_special_cases import LOGLIK_SHAPES

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

SHAPES = LOGLIK_SHAPES
U = 2.0 ** -24
TINY = 2.0 ** -126      # the smallest normal float32
STD = 0.3
LOG2PI = math.log(2.0 * math.pi)
LOGVAR = float(np.float32(2.0 * math.log(STD)))
INV_VAR = float(np.float32(math.exp(-2.0 * math.log(STD))))


def _lanes(N):
    L = 1
    while 2 * L <= 32 and 2 * L * N <= 256:
        L *= 2
    return L


def _lse_slack(amax, N, depth):
    return U * (2 * np.abs(amax) + 11 * math.log(N) + depth + 16)


def _reference(x, y, m, lw, gl, gb, norm, ops=False):
    """Everything the float64 formulas give for x (G, N, V), y, m (G, V), lw, gl (G, N), gb (G,), with the bounds of the module
    docstring (ops: those of the float32 tensor-op statement)."""
    G, N, V = x.shape
    L = _lanes(N)
    Dd = V if ops else -(-V // L) + int(math.log2(L))
    obs = m != 0
    with np.errstate(invalid='ignore'):
        d = np.where(obs[:, None], y[:, None] - x, 0.0)
    mm = np.where(obs, m, 0.0)
    Q, C = (mm[:, None] * d * d).sum(-1), mm.sum(-1)                       # (G, N), (G,)
    K = LOG2PI + LOGVAR
    lp, A = -0.5 * (K * C[:, None] + INV_VAR * Q), 0.5 * (abs(K) * C[:, None] + INV_VAR * Q)
    E = ((V + 10) if ops else (Dd + 6)) * U * A + U * (LOG2PI + abs(LOGVAR)) * C[:, None]
    div = np.where(C > 0, C, 1.0)[:, None]
    if norm:
        lp, E = np.where(C[:, None] > 0, lp / div, 0.0), (E + (Dd + 2) * U * A) / div
    a = lp + lw
    amax = a.max(1)
    ex = np.exp(a - amax[:, None])
    lse = amax + np.log(ex.sum(1))
    p = ex / ex.sum(1, keepdims=True)
    Ea = E + U * np.abs(a)
    Eb = Ea.max(1) + _lse_slack(amax, N, N if ops else -(-N // 64))
    e = d.mean(1)
    abar = np.abs(d).mean(1)
    Dc = -(-V // min(64 * L, 256)) + 9
    Es = U * ((2 * N + 4) * (mm * np.abs(e) * abar).sum(-1) + (Dc + 4) * (mm * e * e).sum(-1))
    out = dict(logpx=lp, E_logpx=E, count=C, E_count=max(Dd, 1) * U * C, bound=lse - math.log(N), E_bound=Eb,
               sqerr=(mm * e * e).sum(-1), E_sqerr=Es, obs=obs)
    R = np.expm1(2 * (Ea + U * np.abs(a - amax[:, None])).max(1)) + 16 * U      # (G,)
    scale = INV_VAR / (div if norm else 1.0)                                      # (G, 1) or scalar
    md = mm[:, None] * d                                                          # (G, N, V)
    for name, l, b in (('bound', 0 * gl, gb), ('logpx', gl, 0 * gb), ('both', gl, gb)):
        bp = b[:, None] * p
        c = (l + bp) * scale
        gx = c[..., None] * md
        flush = np.abs(b)[:, None] * TINY + TINY      # (p_n, then gb p_n)
        Ex = ((np.abs(bp) * R[:, None] + flush + (np.abs(l) + np.abs(bp)) * (Dd + 10) * U) * scale)[..., None] * np.abs(md) + TINY
        out['via_' + name] = dict(gx=gx, E_gx=Ex, gy=-gx.sum(1), E_gy=Ex.sum(1) + N * U * np.abs(gx).sum(1), gw=bp,
                                  E_gw=np.abs(bp) * (R[:, None] + 2 * U) + flush)
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs in the solve's layout - ys (outer, G N, W), target and mask (outer, G, W) - with NaN in target and ys wherever the
    mask is 0, and the float64 references (norm off and on) on the (G, N, V) view.  Never modified."""
    G, N, O, W = shape
    rng = np.random.default_rng(G + 7 * N + 31 * O + 101 * W)
    y = rng.standard_normal((O, G, W)).astype(np.float32)
    x = (y[:, :, None, :] + 0.4 * rng.standard_normal((O, G, N, W))).astype(np.float32)
    m = (rng.random((O, G, W)) > 0.4).astype(np.float32)
    if G >= 2:
        m[:, 0], m[:, 1] = 0.0, 1.0
    if shape == (3, 5, 2, 3):
        m *= (0.25 + rng.random((O, G, W))).astype(np.float32)      # fractional weights
    y[m == 0] = np.nan
    x[np.broadcast_to((m == 0)[:, :, None, :], x.shape)] = np.nan
    lw = (0.5 * rng.standard_normal((G, N))).astype(np.float32)
    gl, gb = rng.standard_normal((G, N)).astype(np.float32), rng.standard_normal(G).astype(np.float32)
    f = lambda t: t.astype(np.float64)
    xv, yv, mv = f(x).transpose(1, 2, 0, 3).reshape(G, N, O * W), f(y).transpose(1, 0, 2).reshape(G, O * W), f(m).transpose(1, 0, 2).reshape(G, O * W)
    out = dict(x=x.reshape(O, G * N, W), y=y, m=m, lw=lw, gl=gl, gb=gb)
    for norm in (False, True):
        out[norm] = _reference(xv, yv, mv, f(lw), f(gl), f(gb), norm)
    return out


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


def _view(t, shape):
    """(outer, G N, W) on the device -> (G, N, V) float64 numpy"""
    G, N, O, W = shape
    return _np(t).reshape(O, G, N, W).transpose(1, 2, 0, 3).reshape(G, N, O * W)


def _plane(t, shape):
    G, N, O, W = shape
    return _np(t).transpose(1, 0, 2).reshape(G, O * W)


def _ratio(err, bound):
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_against_float64(shape, norm):
    """logpx, count, bound and sqerr within the bounds the module docstring derives; two launches give the same bits; the fully
    masked group gives logpx = 0, count = 0, sqerr = 0 and bound = logsumexp(logw) - log N."""
    G, N, O, W = shape
    c = _case(shape)
    r = c[norm]
    args = (_dev(c['x']), N, _dev(c['y']), _dev(c['m']))
    out = S.sample_loglik(*args, std=STD, log_weight=_dev(c['lw']), norm=norm, stats=True)
    bound, logpx, count, sqerr = out
    assert tuple(logpx.shape) == (G, N) and tuple(bound.shape) == tuple(count.shape) == tuple(sqerr.shape) == (G,)
    assert all(t.dtype == torch.float32 for t in out) and all(bool(torch.isfinite(t).all()) for t in out)
    ratios = {k: _ratio(np.abs(_np(t) - r[k]), r['E_' + k]) for k, t in (('logpx', logpx), ('count', count), ('bound', bound), ('sqerr', sqerr))}
    print(f'sample_loglik {shape} norm={norm}: err / bound max ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    for a, b in zip(S.sample_loglik(*args, std=STD, log_weight=_dev(c['lw']), norm=norm, stats=True), out):
        assert torch.equal(a, b)
    assert torch.equal(S.sample_loglik(*args, std=STD, log_weight=_dev(c['lw']), norm=norm), bound)
    if shape != (3, 5, 2, 3):      # (0 / 1 masks: mask=None reads the same mask off the NaN marks)
        assert torch.equal(S.sample_loglik(_dev(c['x']), N, _dev(c['y']), std=STD, log_weight=_dev(c['lw']), norm=norm), bound)
    if G >= 2:
        assert float(logpx[0].abs().max()) == 0 and float(count[0]) == 0 and float(sqerr[0]) == 0
        assert float(count[1]) == O * W or shape == (3, 5, 2, 3)      # (fully observed; with fractional weights their sum)
        nolw = S.sample_loglik(*args, std=STD, norm=norm)
        assert abs(float(nolw[0])) <= _lse_slack(0.0, N, -(-N // 64))


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_gradients_against_the_float64_formulas(shape, norm):
    """grad_ys, grad_target and grad_logw with the gradient arriving through bound alone, through logpx alone and through both;
    exact zeros at every unobserved element (which holds NaN in both inputs)."""
    G, N, O, W = shape
    c = _case(shape)
    r = c[norm]
    hidden_y = _dev(c['m']) == 0
    hidden_x = hidden_y.repeat_interleave(N, dim=1)
    gl, gb = _dev(c['gl']), _dev(c['gb'])
    for name in ('bound', 'logpx', 'both'):
        xd, yd, lwd = _dev(c['x']).requires_grad_(True), _dev(c['y']).requires_grad_(True), _dev(c['lw']).requires_grad_(True)
        bound, logpx, count, sqerr = S.sample_loglik(xd, N, yd, _dev(c['m']), std=STD, log_weight=lwd, norm=norm, stats=True)
        assert type(bound.grad_fn).__name__.startswith('_SampleLoglik') and not count.requires_grad and not sqerr.requires_grad
        outs, gs = {'bound': ((bound,), (gb,)), 'logpx': ((logpx,), (gl,)), 'both': ((bound, logpx), (gb, gl))}[name]
        gx, gy, gw = torch.autograd.grad(outs, (xd, yd, lwd), gs)
        assert all(bool(torch.isfinite(t).all()) for t in (gx, gy, gw))
        assert bool((gx[hidden_x] == 0).all()) and bool((gy[hidden_y] == 0).all())
        want = r['via_' + name]
        ratios = dict(grad_ys=_ratio(np.abs(_view(gx, shape) - want['gx']), want['E_gx']),
                      grad_target=_ratio(np.abs(_plane(gy, shape) - want['gy']), want['E_gy']),
                      grad_logw=_ratio(np.abs(_np(gw) - want['gw']), want['E_gw']))
        print(f'sample_loglik backward {shape} norm={norm} through {name}: err / bound max ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), (name, ratios)
        if name == 'both':
            # engine.sample_loglik_backward: the same launch without autograd, and again: the same bits
            for _ in range(2):
                hx, hy, hw = engine.sample_loglik_backward(gl, gb, xd.detach(), yd.detach(), _dev(c['m']), logpx.detach(), count, N, std=STD,
                                                           log_weight=lwd.detach(), norm=norm)
                assert torch.equal(hx, gx) and torch.equal(hy, gy) and torch.equal(hw, gw)
            # only ys requires grad: grad_target and grad_logw are not asked for
            x2 = xd.detach().requires_grad_(True)
            o2 = S.sample_loglik(x2, N, yd.detach(), _dev(c['m']), std=STD, log_weight=lwd.detach(), norm=norm, stats=True)
            assert torch.equal(torch.autograd.grad(o2[:2], x2, (gb, gl))[0], gx)


def test_off_domain_inputs_take_the_tensor_op_route():
    """On the kernels' domain the native route and the tensor-op statement on the same device agree within the sum of both
    bounds; N = 257 and float64 run the tensor-op statement (within its own bound of float64 / to float64 accuracy)."""
    shape = (2, 7, 3, 130)
    G, N, O, W = shape
    c = _case(shape)
    for norm in (False, True):
        r = c[norm]
        x, y, m, lw = (_dev(c[k]) for k in ('x', 'y', 'm', 'lw'))
        f = lambda t: t.astype(np.float64)
        ro = _reference(f(c['x']).reshape(O, G, N, W).transpose(1, 2, 0, 3).reshape(G, N, O * W), f(c['y']).transpose(1, 0, 2).reshape(G, O * W),
                        f(c['m']).transpose(1, 0, 2).reshape(G, O * W), f(c['lw']), f(c['gl']), f(c['gb']), norm, ops=True)
        a = S.sample_loglik(x, N, y, m, std=STD, log_weight=lw, norm=norm, stats=True)
        b = engine.sample_loglik_tensor_ops(x, N, y, m, std=STD, log_weight=lw, norm=norm, stats=True)
        for k, u, v in zip(('bound', 'logpx', 'count', 'sqerr'), a, b):
            assert _ratio(np.abs(_np(u) - _np(v)), r['E_' + k] + ro['E_' + k]) <= 1.0, k
            assert _ratio(np.abs(_np(v) - ro[k]), ro['E_' + k]) <= 1.0, k
        x64 = x.double().requires_grad_(True)
        o64 = S.sample_loglik(x64, N, y.double(), m.double(), std=STD, log_weight=lw.double(), norm=norm, stats=True)
        assert o64[0].dtype == torch.float64 and not type(o64[0].grad_fn).__name__.startswith('_SampleLoglik')
        # (the references use the float32 variance the kernel receives, the float64 route the exact one: 2^-24 relatively apart)
        assert float((o64[1].detach().cpu() - torch.from_numpy(r['logpx'])).abs().max()) <= 1e-6 * float(np.abs(r['logpx']).max())
    N2, G2, W2 = 257, 2, 3
    gen = torch.Generator().manual_seed(5)
    y2 = torch.randn(G2, W2, generator=gen)
    x2 = (y2[:, None] + 0.4 * torch.randn(G2, N2, W2, generator=gen)).reshape(G2 * N2, W2)
    m2 = torch.tensor([[1.0, 0.0, 1.0], [1.0, 1.0, 0.5]])
    y2[0, 1] = float('nan')
    xd = x2.to(DEV).requires_grad_(True)
    out = S.sample_loglik(xd, N2, y2.to(DEV), m2.to(DEV), std=STD, stats=True)
    assert out[0].grad_fn is not None and not type(out[0].grad_fn).__name__.startswith('_SampleLoglik')
    ro = _reference(x2.double().numpy().reshape(G2, N2, W2), y2.double().numpy(), m2.double().numpy(), np.zeros((G2, N2)), np.zeros((G2, N2)),
                    np.zeros(G2), False, ops=True)
    for k, t in zip(('bound', 'logpx', 'count', 'sqerr'), out):
        assert _ratio(np.abs(_np(t) - ro[k]), ro['E_' + k]) <= 1.0, k
    gx, = torch.autograd.grad(out[0].sum(), xd)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0 and float(gx[:N2, 1].abs().max()) == 0


def test_special_values_stay_in_their_own_group():
    """A NaN at an observed element of one path poisons that path's logpx and its group's bound and sqerr; a path at +Inf has
    logpx = -Inf and leaves the bound finite; the classes (finite, +-Inf, NaN) are those of the float64 statement.  The backward
    of the untouched group has the bits of the call without the special values."""
    G, N, W = 3, 4, 70
    gen = torch.Generator().manual_seed(11)
    y = torch.randn(G, W, generator=gen)
    x = (y[:, None] + 0.4 * torch.randn(G, N, W, generator=gen)).reshape(G * N, W)
    m = (torch.rand(G, W, generator=gen) > 0.4).float()
    m[:, 3] = m[:, 69] = 1.0
    clean = x.clone()
    x[N + 2, 3] = float('nan')
    x[2 * N + 1, 69] = float('inf')
    for norm in (False, True):
        out = S.sample_loglik(x.to(DEV), N, y.to(DEV), m.to(DEV), std=STD, norm=norm, stats=True)
        ref = engine.sample_loglik_tensor_ops(x.double(), N, y.double(), m.double(), std=STD, norm=norm, stats=True)
        for k, a, b in zip(('bound', 'logpx', 'count', 'sqerr'), out, ref):
            a = a.cpu()
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a == float('inf'), b == float('inf')), k
            assert torch.equal(a == -float('inf'), b == -float('inf')), k
        bound, logpx, count, sqerr = (t.cpu() for t in out)
        assert bool(torch.isnan(logpx[1, 2])) and int(torch.isnan(logpx).sum()) == 1 and bool(torch.isnan(bound[1])) and bool(torch.isnan(sqerr[1]))
        assert float(logpx[2, 1]) == -float('inf') and bool(torch.isfinite(bound[2])) and bool(torch.isfinite(bound[0]))
        grads = []
        for src in (x, clean):
            xd, yd = src.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
            o = S.sample_loglik(xd, N, yd, m.to(DEV), std=STD, norm=norm, stats=True)
            gx, gy = torch.autograd.grad(o[0][0] + o[1][0].sum(), (xd, yd))
            grads.append((gx[:N], gy[0], o[0][0].detach(), o[1][0].detach()))
        for a, b in zip(grads[0], grads[1]):
            assert torch.equal(a, b)
        assert float(grads[0][0].abs().max()) > 0 and bool(torch.isfinite(grads[0][0]).all())


def test_pooled_ensemble_layout_gives_the_bits_of_the_permuted_single_member_call():
    O, M, G, Sn, W = 2, 2, 5, 4, 70
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(O, M, G * Sn, W, generator=gen)
    y = torch.randn(O, G, W, generator=gen)
    m = (torch.rand(O, G, W, generator=gen) > 0.4).float() * (0.5 + torch.rand(O, G, W, generator=gen))
    y[m == 0] = float('nan')
    lw, gl, gb = torch.randn(G, M * Sn, generator=gen), torch.randn(G, M * Sn, generator=gen), torch.randn(G, generator=gen)
    flat = x.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W).contiguous()
    for norm in (False, True):
        xa, xb, ya, yb, la, lb = (t.to(DEV).requires_grad_(True) for t in (x, flat, y, y, lw, lw))
        a = S.sample_loglik(xa, Sn, ya, m.to(DEV), std=STD, members=M, log_weight=la, norm=norm, stats=True)
        b = S.sample_loglik(xb, M * Sn, yb, m.to(DEV), std=STD, log_weight=lb, norm=norm, stats=True)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        assert tuple(a[1].shape) == (G, M * Sn) and bool(torch.isfinite(a[0]).all())
        ga = torch.autograd.grad(a[:2], (xa, ya, la), (gb.to(DEV), gl.to(DEV)))
        gb_ = torch.autograd.grad(b[:2], (xb, yb, lb), (gb.to(DEV), gl.to(DEV)))
        assert torch.equal(ga[0].reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), gb_[0])
        assert torch.equal(ga[1], gb_[1]) and torch.equal(ga[2], gb_[2]) and float(ga[0].abs().max()) > 0


def test_unaligned_and_non_contiguous_inputs_give_the_bits_of_their_clones():
    G, N, W = 4, 6, 37
    buf, tb = torch.randn(G * N * W + 1, device=DEV), torch.randn(G * W + 1, device=DEV)
    mb = (torch.rand(G * W + 1, device=DEV) > 0.4).float()
    xu, tu, mu = buf[1:].reshape(G * N, W).requires_grad_(True), tb[1:].reshape(G, W), mb[1:].reshape(G, W)      # 4 bytes off a 16-byte boundary
    xc, tc, mc = buf[1:].clone().reshape(G * N, W).requires_grad_(True), tu.clone(), mu.clone()
    a, b = S.sample_loglik(xu, N, tu, mu, stats=True), S.sample_loglik(xc, N, tc, mc, stats=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(torch.autograd.grad(a[0].sum(), xu)[0], torch.autograd.grad(b[0].sum(), xc)[0])
    wide = torch.randn(G * N, 2 * W, device=DEV).requires_grad_(True)
    xs = wide[:, ::2]
    xk = xs.detach().clone().requires_grad_(True)
    c1, c2 = S.sample_loglik(xs, N, tu, mu), S.sample_loglik(xk, N, tu, mu)
    assert not xs.is_contiguous() and torch.equal(c1, c2)
    g1, g2 = torch.autograd.grad(c1.sum(), wide)[0], torch.autograd.grad(c2.sum(), xk)[0]
    assert torch.equal(g1[:, ::2], g2) and float(g1[:, 1::2].abs().max()) == 0


TIMES = np.array([0., 1., 2., 3., 4., 5.], np.float32)


def test_a_model_trains_on_iwae_loss_through_a_graphed_step_with_a_nan_marked_target():
    Sn, B, H, Cn, out_time = 2, 4, 64, 3, 2
    pr = make_problem(31, 4, 17, 2, B, H, Cn, len(TIMES), times=TIMES)
    torch.manual_seed(700)
    func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=17)
    model = S.NeuralSDE_forecasting(func, Cn, out_time, H, Cn).to(DEV).train()
    model2 = copy.deepcopy(model)
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    true = np.random.default_rng(4).standard_normal((B, out_time, Cn)).astype(np.float32)
    true[0, 1, 2] = true[2, 0, 0] = true[3, 1, 1] = np.nan
    true = torch.from_numpy(true).to(DEV)
    lengths = torch.full((B,), len(TIMES) - 1, device=DEV)
    kwargs = {'method': 'euler', 'options': {'seed': 9, 'samples': Sn, 'sample_grad': True}}
    base = S.iwae_loss(Sn, std=0.5)
    seen = []

    def loss_fn(pred, y):
        assert tuple(pred.shape) == (B * Sn, out_time, Cn)
        loss = base(pred, y)
        seen.append(loss.detach())      # (under capture: a view of the recording's loss, refreshed by every replay)
        return loss

    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    for _ in range(2):
        loss_fn(model(times, (coeffs,), lengths, **kwargs), true).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    eager = [t.clone() for t in seen]
    del seen[:]
    opt2 = torch.optim.Adam(model2.parameters(), lr=1e-3, capturable=True)
    graphed = train.GraphedStep(model2, times, opt2, loss_fn, kwargs, torch.device(DEV), warmup=1)
    graphed((coeffs,), true, lengths)      # the warm-up step of this batch shape: eager
    graphed((coeffs,), true, lengths)      # recorded, then replayed
    torch.cuda.synchronize()
    assert graphed.disabled is None and graphed.replays == 1, graphed.disabled
    assert len(seen) == 2 and torch.equal(seen[0], eager[0]) and torch.equal(seen[1], eager[1])
    assert bool(torch.isfinite(eager[1])) and not torch.equal(eager[0], eager[1])
    for p, p2 in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, p2) and bool(torch.isfinite(p).all())
