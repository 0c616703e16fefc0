"""snsde_sample_loglik_noise, its adjoint and the per-channel reduce on the GPU, through sample_loglik(log_std=) / iwae_loss(noise=).

Shapes (groups G, pooled samples N, outer, width W), V = outer W.  The buckets follow from N alone, as for the scalar kernel
(tests/test_gpu_sample_loglik.py): L = min(32, largest power of two <= 256 / N) lanes per sample, chunks of CW = 64 L columns,
RS = max(1, 4 / L) row parts.  N = 1, 2, 3, 8 (L = 32, CW = 2048), 9 (L = 16, CW = 1024), 64 (L = 4, CW = 256), 65 (L = 2, CW = 128,
RS = 2), 255 and 256 (L = 1, CW = 64, RS = 4), each with V exactly at its chunk width and exactly one past it (2049 = 3 x 683,
1025 = 5 x 205, 129 = 3 x 43, 65 = 5 x 13); most "one past" shapes take V from outer > 1 slices of a width that is no multiple
of 4, so a chunk straddles an outer boundary and the channel v mod W wraps inside it; (3, 5, 2, 3) carries fractional mask
weights.  With SNSDE_LOGLIK_NOISE_MARGINS set, every printed ratio line is also appended to that file
(profiles/sample_loglik_noise_margins.txt is such a run).  Where G >= 2, group 0 is fully masked and group 1 observed wherever
its channel is; where W >= 3, channel 0 is fully masked.  target, ys AND log_std (the per-entry plane at every unobserved entry,
the per-channel vector at the fully masked channel) hold NaN where nothing is observed.  The float64 reference is the tensor-op
statement (engine.sample_loglik_tensor_ops) on the float32 inputs in float64, values and autograd gradients, once per shape.

The bounds, u = 2^-24, from the summation order include/snsde.h documents; Dd = ceil(V / L) + log2 L is the depth of a sub-lane's
chain plus the butterfly; expf and logf are taken within 2 ulp = 4 u, as in the scalar test.
  logpx = -1/2 (q_n + lv).  q_n = sum u_v d^2: d = y - x rounds once (d^2: 2 u), iv_v = expf(-2 ls_v) 4 u (the product -2 ls is
  exact), u_v = m_v iv_v once, u_v d once, the fmaf chain and butterfly Dd: q_n within (Dd + 9) u q_n.  lv = sum t_v, t_v = m_v
  fmaf(2, ls_v, (float)log 2 pi): the constant is off by u log 2 pi, the fmaf and the product round once each, the chain Dd: within
  (Dd + 2) u T + u log 2 pi count, T = sum m_v |2 ls_v + log 2 pi|.  The closing addition rounds once.  With A_n = (q_n + T) / 2:
  |err| <= (Dd + 11) u A_n + u log 2 pi count; under norm the division and count add (Dd + 2) u A_n, all over count.
  count within Dd u count; bound and sqerr: the scalar test's E_lse and E_sqerr (the same code).
  backward: p_n relatively within R = expm1(2 max_n E'_n) + 16 u as there.  c_n = (gl_n + gb p_n) / count: an addition and a
  division.  grad_ys = (c_n u_v) d: u_v 5 u, c_n 2 u, the two products 2 u, d u: |err| <= (|gb| p_n R + (|gl_n| + |gb| p_n) 12 u)
  / count u_v |d|; grad_target adds these over n plus N u sum_n |grad_ys|; grad_logw = gb p_n within |gb| p_n (R + 2 u).
  grad_log_std[v] = m_v sum_n c_n z_n, z_n = fmaf(d iv, d, -1): d^2 2 u, iv 4 u, d iv once, the fmaf once: z_n within 8 u (d^2 iv
  + 1); the chain of N fmafs and the product with m_v: |err| <= m_v sum_n [cerr_n |z_n| + (N + 10) u cabs_n (d^2 iv + 1)], cabs_n
  = (|gl_n| + |gb| p_n) / count, cerr_n = (|gb| p_n R + 2 u (|gl_n| + |gb| p_n)) / count.  The per-channel gradient adds the bounds
  of its rows and (min(rows, 64) + ceil(rows / 64)) u sum_rows |grad_log_std| for the two-stage sum.
  TINY = 2^-126 enters as in the scalar test (p_n flushed to zero far below the best path).
The tensor-op statement in float32 (the routing test): (V + 12) u A_n + u log 2 pi count, and E_lse with N in place of
ceil(N / 64)."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine, train
from tests.buffer_arena import same_bits
from tests.helpers import make_problem
from tests.kernel_cases import STEP_OFFSET_CASES
from tests.test_gpu_buffer_contract import ALIGNMENT_SEEN, run as run_contract
from tests.test_gpu_filter_grad import step_bound

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1, 2048), (2, 1, 3, 683), (2, 2, 1, 2048), (3, 2, 1, 2049), (2, 3, 2, 1024), (2, 3, 3, 683), (3, 5, 2, 3),
          (2, 8, 1, 2048), (2, 8, 3, 683), (2, 9, 1, 1024), (2, 9, 5, 205), (2, 64, 1, 256), (2, 64, 1, 257), (2, 65, 1, 128),
          (2, 65, 3, 43), (2, 255, 1, 64), (1, 255, 1, 65), (2, 256, 1, 64), (2, 256, 5, 13), (8, 12, 2, 37)]      # (G, N, outer, W)
U = 2.0 ** -24
TINY = 2.0 ** -126
LOG2PI = math.log(2.0 * math.pi)
NAN = float('nan')


def _lanes(N):
    L = 1
    while 2 * L <= 32 and 2 * L * N <= 256:
        L *= 2
    return L


def _gnv(t, shape, per_sample):
    """(outer, G [N], W) -> (G, [N,] V)"""
    G, N, O, W = shape
    if per_sample:
        return t.reshape(O, G, N, W).permute(1, 2, 0, 3).reshape(G, N, O * W)
    return t.reshape(O, G, W).permute(1, 0, 2).reshape(G, O * W)


def _lse_slack(amax, N, depth):
    return U * (2 * amax.abs() + 11 * math.log(N) + depth + 16)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """float32 device tensors in the solve's layout; NaN wherever nothing is observed.  Never modified."""
    G, N, O, W = shape
    gen = torch.Generator().manual_seed(G + 7 * N + 31 * O + 101 * W)
    y = torch.randn(O, G, W, generator=gen)
    x = y[:, :, None, :] + 0.4 * torch.randn(O, G, N, W, generator=gen)
    m = (torch.rand(O, G, W, generator=gen) > 0.4).float()
    if G >= 2:
        m[:, 0], m[:, 1] = 0.0, 1.0
    if W >= 3:
        m[:, :, 0] = 0.0
    if shape == (3, 5, 2, 3):
        m *= 0.25 + torch.rand(O, G, W, generator=gen)
    ls_c = 0.4 * torch.randn(W, generator=gen) - 0.7
    ls_e = ls_c + 0.3 * torch.randn(O, G, W, generator=gen)
    y[m == 0] = NAN
    x[(m == 0)[:, :, None, :].expand_as(x)] = NAN
    ls_e[m == 0] = NAN
    ls_c[(m == 0).reshape(-1, W).all(0)] = NAN
    lw, gl, gb = 0.5 * torch.randn(G, N, generator=gen), torch.randn(G, N, generator=gen), torch.randn(G, generator=gen)
    out = dict(x=x.reshape(O, G * N, W), y=y, m=m, ls_c=ls_c, ls_e=ls_e, lw=lw, gl=gl, gb=gb)
    return {k: v.contiguous().to(DEV) for k, v in out.items()}


VIA = ('bound', 'logpx', 'both')


@functools.lru_cache(maxsize=None)
def _reference(shape, entry, norm, ops=False):
    """The float64 tensor-op statement on the float32 inputs - values and, for the gradient arriving through bound, through logpx
    and through both, the four gradients - with the bounds of the module docstring (ops: of the float32 tensor-op statement)."""
    G, N, O, W = shape
    V = O * W
    c = _inputs(shape)
    L = _lanes(N)
    Dd = V if ops else -(-V // L) + int(math.log2(L))
    x, y, lw, ls = (c[k].double().requires_grad_(True) for k in ('x', 'y', 'lw', 'ls_e' if entry else 'ls_c'))
    m, gl, gb = c['m'].double(), c['gl'].double(), c['gb'].double()
    bound, logpx, count, sqerr = engine.sample_loglik_tensor_ops(x, N, y, m, log_weight=lw, norm=norm, stats=True, log_std=ls)
    out = dict(bound=bound.detach(), logpx=logpx.detach(), count=count.detach(), sqerr=sqerr.detach())
    for via in VIA:
        outs, gs = {'bound': ((bound,), (gb,)), 'logpx': ((logpx,), (gl,)), 'both': ((bound, logpx), (gb, gl))}[via]
        gr = torch.autograd.grad(outs, (x, y, lw, ls), gs, retain_graph=True, allow_unused=True)      # (logpx does not depend on lw)
        out['via_' + via] = {k: torch.zeros_like(t) if g is None else g for k, g, t in zip(('gx', 'gy', 'gw', 'gls'), gr, (x, y, lw, ls))}
    # the magnitudes of the bounds, on the (G, N, V) view
    with torch.no_grad():
        xv, yv, mv = _gnv(x, shape, True), _gnv(y, shape, False), _gnv(m, shape, False)
        lsv = _gnv(ls if entry else ls.expand(O, G, W), shape, False)
        obs = mv != 0
        zero = xv.new_zeros(())
        d = torch.where(obs[:, None], yv[:, None] - xv, zero)
        lz = torch.where(obs, lsv, zero)
        iv = torch.exp(-2.0 * lz)
        uv = mv * iv                                                            # (G, V)
        Q = (uv[:, None] * d * d).sum(-1)                                       # (G, N)
        T = (mv * (2.0 * lz + LOG2PI).abs()).sum(-1)                            # (G,)
        C = mv.sum(-1)
        A = 0.5 * (Q + T[:, None])
        E = ((V + 12) if ops else (Dd + 11)) * U * A + U * LOG2PI * C[:, None]
        div = torch.where(C > 0, C, torch.ones_like(C))[:, None]
        if norm:
            E = (E + (Dd + 2) * U * A) / div
        a = out['logpx'] + lw
        amax = a.max(1).values
        p = torch.softmax(a, dim=1)
        Ea = E + U * a.abs()
        out['E_logpx'], out['E_count'] = E, max(Dd, 1) * U * C
        out['E_bound'] = Ea.max(1).values + _lse_slack(amax, N, N if ops else -(-N // 64))
        e, abar = d.mean(1), d.abs().mean(1)
        Dc = -(-V // min(64 * L, 256)) + 9
        out['E_sqerr'] = U * ((2 * N + 4) * (mv * e.abs() * abar).sum(-1) + (Dc + 4) * (mv * e * e).sum(-1))
        R = torch.expm1(2 * (Ea + U * (a - amax[:, None]).abs()).max(1).values) + 16 * U      # (G,)
        scale = 1.0 / div if norm else torch.ones_like(div)
        ud = uv[:, None] * d.abs()                                              # (G, N, V)
        z, zabs = d * d * iv[:, None] - 1.0, d * d * iv[:, None] + 1.0
        rows = O * G
        for via, l, b in (('bound', 0 * gl, gb), ('logpx', gl, 0 * gb), ('both', gl, gb)):
            bp = (b[:, None] * p).abs()
            flush = b.abs()[:, None] * TINY + TINY
            cabs = (l.abs() + bp) * scale
            cerr = (bp * R[:, None] + flush + 2 * U * (l.abs() + bp)) * scale
            r = out['via_' + via]
            Ex = (cerr + 10 * U * cabs)[..., None] * ud + TINY
            r['E_gx'] = Ex
            r['E_gy'] = Ex.sum(1) + N * U * _gnv(r['gx'], shape, True).abs().sum(1)
            r['E_gw'] = bp * (R[:, None] + 2 * U) + flush
            Ee = mv * (cerr[..., None] * z.abs() + (N + 10) * U * cabs[..., None] * zabs).sum(1) + TINY      # (G, V), 0 where unobserved
            Ee = torch.where(obs, Ee, zero)
            if entry:
                r['E_gls'] = Ee
            else:      # (sum over the rows (o, g) of the plane)
                gabs = mv * (((l + b[:, None] * p) * scale)[..., None] * z).sum(1).abs()      # |entry gradient|, (G, V)
                fold = lambda t: t.reshape(G, O, W).sum((0, 1))
                r['E_gls'] = fold(Ee) + (min(rows, 64) + -(-rows // 64)) * U * fold(gabs) + TINY
    return out


def _report(line):
    print(line)
    if os.environ.get('SNSDE_LOGLIK_NOISE_MARGINS'):
        with open(os.environ['SNSDE_LOGLIK_NOISE_MARGINS'], 'a') as fh:
            fh.write(line + '\n')


def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), r)
    return float(r.max())


def _call(c, N, entry, norm, grad=False, **kw):
    t = {k: (c[k].clone().requires_grad_(True) if grad and k in ('x', 'y', 'lw', 'ls') else c[k]) for k in ('x', 'y', 'm', 'lw')}
    ls = c['ls_e' if entry else 'ls_c']
    ls = ls.clone().requires_grad_(True) if grad else ls
    out = S.sample_loglik(t['x'], N, t['y'], t['m'], log_weight=t['lw'], norm=norm, stats=True, log_std=ls, **kw)
    return out, (t['x'], t['y'], t['lw'], ls)


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_gradients_against_float64_in_both_modes(shape, norm):
    """Forward and the four gradients (through bound, through logpx, through both) of both modes within the derived bounds (the
    worst ratio per quantity is printed); the same bits on a second launch; exact zeros at every unobserved element, which holds
    NaN in ys, target and log_std; the fully masked group gives logpx = count = sqerr = 0."""
    G, N, O, W = shape
    c = _inputs(shape)
    hidden = c['m'] == 0
    hidden_x = hidden.repeat_interleave(N, dim=1)
    for entry in (False, True):
        r = _reference(shape, entry, norm)
        out, leaves = _call(c, N, entry, norm, grad=True)
        bound, logpx, count, sqerr = out
        assert type(bound.grad_fn).__name__ == '_SampleLoglikNoiseBackward' and not count.requires_grad and not sqerr.requires_grad
        assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in out)
        ratios = {k: _ratio(t.detach(), r[k], r['E_' + k]) for k, t in zip(('bound', 'logpx', 'count', 'sqerr'), out)}
        for a, b in zip(_call(c, N, entry, norm)[0], out):      # the launch outside autograd, again: the same bits
            assert torch.equal(a, b.detach())
        if G >= 2:
            assert float(logpx.detach()[0].abs().max()) == 0 and float(count[0]) == 0 and float(sqerr[0]) == 0
        for via in VIA:
            outs, gs = {'bound': ((bound,), (c['gb'],)), 'logpx': ((logpx,), (c['gl'],)), 'both': ((bound, logpx), (c['gb'], c['gl']))}[via]
            gx, gy, gw, gls = torch.autograd.grad(outs, leaves, gs, retain_graph=True)
            assert all(bool(torch.isfinite(t).all()) for t in (gx, gy, gw, gls))
            assert bool((gx[hidden_x] == 0).all()) and bool((gy[hidden] == 0).all())
            if entry:
                assert bool((gls[hidden] == 0).all()) and not bool(torch.signbit(gls[hidden]).any())
            elif W >= 3:
                assert float(gls[0]) == 0
            w = r['via_' + via]
            ratios.update({f'{via}:grad_ys': _ratio(_gnv(gx, shape, True), _gnv(w['gx'], shape, True), w['E_gx']),
                           f'{via}:grad_target': _ratio(_gnv(gy, shape, False), _gnv(w['gy'], shape, False), w['E_gy']),
                           f'{via}:grad_logw': _ratio(gw, w['gw'], w['E_gw']),
                           f'{via}:grad_log_std': _ratio(_gnv(gls, shape, False) if entry else gls, _gnv(w['gls'], shape, False) if entry else w['gls'],
                                                         w['E_gls'])})
        _report(f'sample_loglik_noise {shape} norm={int(norm)} {"entry" if entry else "channel"}: err / bound max '
                + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
        assert all(v < 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_channel_mode_has_the_bits_of_entry_mode_and_of_the_documented_reduction(shape):
    """(a) channel mode = entry mode on the broadcast plane, values and grad_ys (and grad_target, grad_logw), and count = the
    scalar kernel's count, bit for bit; (b) the channel
    gradient = the reduce entry point on the entry-mode gradient = the documented order written out: blocks of 64 rows, each
    ascending, then the blocks ascending."""
    G, N, O, W = shape
    c = dict(_inputs(shape))
    c['ls_e'] = c['ls_c'].expand(O, G, W).contiguous()
    for norm in (False, True):
        oc, lc = _call(c, N, False, norm, grad=True)
        oe, le = _call(c, N, True, norm, grad=True)
        for a, b in zip(oc, oe):
            assert torch.equal(a, b)
        # count (and sqerr, which the noise does not weigh) run the scalar kernel's chains: its bits, fractional mask weights included
        scalar = S.sample_loglik(c['x'], N, c['y'], c['m'], std=0.3, log_weight=c['lw'], norm=norm, stats=True)
        assert torch.equal(scalar[2], oc[2]) and torch.equal(scalar[3], oc[3])
        gc = torch.autograd.grad(oc[:2], lc, (c['gb'], c['gl']))
        ge = torch.autograd.grad(oe[:2], le, (c['gb'], c['gl']))
        for a, b in zip(gc[:3], ge[:3]):
            assert torch.equal(a, b)
        assert torch.equal(gc[3], engine.sample_loglik_noise_reduce(ge[3]))
        rows = ge[3].reshape(O * G, W)
        parts = []
        for k in range(0, O * G, _lib.LOGLIK_NOISE_REDUCE_ROWS):
            s = rows[k].clone()
            for row in rows[k + 1:k + _lib.LOGLIK_NOISE_REDUCE_ROWS]:
                s = s + row
            parts.append(s)
        total = parts[0]
        for s in parts[1:]:
            total = total + s
        assert torch.equal(gc[3], total)
        # the launch without autograd (engine.sample_loglik_noise_backward), twice: the same bits
        for _ in range(2):
            h = engine.sample_loglik_noise_backward(c['gl'], c['gb'], c['x'], c['y'], c['m'], c['ls_c'], oc[1].detach(), oc[2], N,
                                                    log_weight=c['lw'], norm=norm)
            assert all(torch.equal(a, b) for a, b in zip(h, gc))


def test_a_0_dim_log_std_is_the_vector_of_that_value():
    """... through autograd (its gradient is the sum over the channels) and through engine.sample_loglik_noise_backward, which is
    handed the stride-0 expansion and must not read it as W adjacent floats."""
    shape = (8, 12, 2, 37)
    G, N, O, W = shape
    c = _inputs(shape)
    s0 = torch.tensor(-0.6, device=DEV, requires_grad=True)
    sv = torch.full((W,), -0.6, device=DEV, requires_grad=True)
    a = S.sample_loglik(c['x'], N, c['y'], c['m'], log_weight=c['lw'], stats=True, log_std=s0)
    b = S.sample_loglik(c['x'], N, c['y'], c['m'], log_weight=c['lw'], stats=True, log_std=sv)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    g0, gv = torch.autograd.grad(a[0].sum(), s0)[0], torch.autograd.grad(b[0].sum(), sv)[0]
    assert g0.shape == () and float((g0 - gv.sum()).abs()) <= 8 * W * U * float(gv.abs().sum())
    gb = torch.ones(G, device=DEV)
    h0 = engine.sample_loglik_noise_backward(None, gb, c['x'], c['y'], c['m'], s0.detach(), b[1].detach(), b[2], N, log_weight=c['lw'])
    hv = engine.sample_loglik_noise_backward(None, gb, c['x'], c['y'], c['m'], sv.detach(), b[1].detach(), b[2], N, log_weight=c['lw'])
    assert all(torch.equal(u, v) for u, v in zip(h0, hv)) and torch.equal(hv[3], gv)


def test_the_reduction_over_many_rows_is_the_documented_order():
    """rows = 200 (four blocks, the last of 8 rows) at a width that is no multiple of the block: the partial plane is used."""
    rows, W = 200, 300
    g = torch.randn(5, rows // 5, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    got = engine.sample_loglik_noise_reduce(g)
    flat = g.reshape(rows, W)
    total = None
    for k in range(0, rows, 64):
        s = flat[k].clone()
        for row in flat[k + 1:k + 64]:
            s = s + row
        total = s if total is None else total + s
    assert torch.equal(got, total) and torch.equal(got, engine.sample_loglik_noise_reduce(g))
    assert float((got.double() - flat.double().sum(0)).abs().max()) <= (64 + 4) * U * float(flat.abs().sum(0).max())


def test_unaligned_and_non_contiguous_inputs_give_the_bits_of_their_clones():
    G, N, O, W = 4, 6, 2, 37
    gen = torch.Generator().manual_seed(6)
    flat = lambda n: torch.randn(n + 1, generator=gen).to(DEV)[1:]      # 4 bytes off a 16-byte boundary
    xu, tu, le = flat(O * G * N * W).reshape(O, G * N, W), flat(O * G * W).reshape(O, G, W), flat(O * G * W).reshape(O, G, W)
    lc, lw = flat(W), flat(G * N).reshape(G, N)
    mu = ((torch.rand(O * G * W + 1, generator=gen) > 0.4).float().to(DEV))[1:].reshape(O, G, W)
    for ls in (lc, le):
        ua = [t.detach().requires_grad_(True) for t in (xu, tu, lw, ls)]
        ca = [t.detach().clone().requires_grad_(True) for t in (xu, tu, lw, ls)]
        assert all(t.data_ptr() % 16 == 4 for t in ua) and all(t.data_ptr() % 16 == 0 for t in ca)
        a = S.sample_loglik(ua[0], N, ua[1], mu, log_weight=ua[2], stats=True, log_std=ua[3])
        b = S.sample_loglik(ca[0], N, ca[1], mu.clone(), log_weight=ca[2], stats=True, log_std=ca[3])
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        for u, v in zip(torch.autograd.grad(a[0].sum() + a[1].sum(), ua), torch.autograd.grad(b[0].sum() + b[1].sum(), ca)):
            assert torch.equal(u, v) and float(u.abs().max()) > 0
    wide = torch.randn(O, G * N, 2 * W, generator=gen).to(DEV).requires_grad_(True)
    lwide = torch.randn(O, G, 2 * W, generator=gen).to(DEV).requires_grad_(True)
    xs, lsn = wide[..., ::2], lwide[..., ::2]
    xk, lk = xs.detach().clone().requires_grad_(True), lsn.detach().clone().requires_grad_(True)
    c1, c2 = S.sample_loglik(xs, N, tu, mu, log_std=lsn), S.sample_loglik(xk, N, tu, mu, log_std=lk)
    assert not xs.is_contiguous() and not lsn.is_contiguous() and torch.equal(c1, c2)
    g1, g2 = torch.autograd.grad(c1.sum(), (wide, lwide)), torch.autograd.grad(c2.sum(), (xk, lk))
    assert torch.equal(g1[0][..., ::2], g2[0]) and torch.equal(g1[1][..., ::2], g2[1]) and float(g1[1][..., 1::2].abs().max()) == 0


def test_pooled_members_give_the_bits_of_the_permuted_single_member_call():
    O, M, G, Sn, W = 2, 2, 5, 4, 70
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(O, M, G * Sn, W, generator=gen)
    y = torch.randn(O, G, W, generator=gen)
    m = (torch.rand(O, G, W, generator=gen) > 0.4).float() * (0.5 + torch.rand(O, G, W, generator=gen))
    y[m == 0] = NAN
    lw, gl, gb = torch.randn(G, M * Sn, generator=gen), torch.randn(G, M * Sn, generator=gen), torch.randn(G, generator=gen)
    flat = x.reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W).contiguous()
    for ls in (0.3 * torch.randn(W, generator=gen) - 0.5, 0.3 * torch.randn(O, G, W, generator=gen) - 0.5):
        for norm in (False, True):
            xa, xb, ya, yb, la, lb, sa, sb = (t.to(DEV).requires_grad_(True) for t in (x, flat, y, y, lw, lw, ls, ls))
            a = S.sample_loglik(xa, Sn, ya, m.to(DEV), members=M, log_weight=la, norm=norm, stats=True, log_std=sa)
            b = S.sample_loglik(xb, M * Sn, yb, m.to(DEV), log_weight=lb, norm=norm, stats=True, log_std=sb)
            for u, v in zip(a, b):
                assert torch.equal(u, v)
            assert tuple(a[1].shape) == (G, M * Sn) and bool(torch.isfinite(a[0]).all())
            ga = torch.autograd.grad(a[:2], (xa, ya, la, sa), (gb.to(DEV), gl.to(DEV)))
            gb_ = torch.autograd.grad(b[:2], (xb, yb, lb, sb), (gb.to(DEV), gl.to(DEV)))
            assert torch.equal(ga[0].reshape(O, M, G, Sn, W).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, W), gb_[0])
            assert all(torch.equal(u, v) for u, v in zip(ga[1:], gb_[1:])) and float(ga[3].abs().max()) > 0


def test_off_domain_inputs_take_the_tensor_op_route():
    """N = 257, float64 and CPU tensors run the tensor-op statement: no _SampleLoglikNoise node, the answer of the float64
    reference within the float32 statement's bound (float64: to float64 accuracy); on the domain the two routes agree within the
    sum of their bounds."""
    shape = (8, 12, 2, 37)
    G, N, O, W = shape
    c = _inputs(shape)
    for entry in (False, True):
        ls = c['ls_e' if entry else 'ls_c']
        for norm in (False, True):
            r, ro = _reference(shape, entry, norm), _reference(shape, entry, norm, ops=True)
            a = S.sample_loglik(c['x'], N, c['y'], c['m'], log_weight=c['lw'], norm=norm, stats=True, log_std=ls)
            b = engine.sample_loglik_tensor_ops(c['x'], N, c['y'], c['m'], log_weight=c['lw'], norm=norm, stats=True, log_std=ls)
            cpu = S.sample_loglik(c['x'].cpu(), N, c['y'].cpu(), c['m'].cpu(), log_weight=c['lw'].cpu(), norm=norm, stats=True, log_std=ls.cpu())
            for k, u, v, w in zip(('bound', 'logpx', 'count', 'sqerr'), a, b, cpu):
                assert _ratio(u, v.double(), r['E_' + k] + ro['E_' + k]) < 1.0, k
                assert _ratio(v, ro[k], ro['E_' + k]) < 1.0 and _ratio(w.to(DEV), ro[k], ro['E_' + k]) < 1.0, k
            x64 = c['x'].double().requires_grad_(True)
            o64 = S.sample_loglik(x64, N, c['y'].double(), c['m'].double(), log_weight=c['lw'].double(), norm=norm, stats=True, log_std=ls.double())
            assert o64[0].dtype == torch.float64 and not type(o64[0].grad_fn).__name__.startswith('_SampleLoglik')
            assert float((o64[1].detach() - r['logpx']).abs().max()) <= 1e-12 * float(r['logpx'].abs().max())
    N2, G2, W2 = 257, 2, 3
    gen = torch.Generator().manual_seed(5)
    y2 = torch.randn(G2, W2, generator=gen)
    x2 = (y2[:, None] + 0.4 * torch.randn(G2, N2, W2, generator=gen)).reshape(G2 * N2, W2)
    m2 = torch.tensor([[1.0, 0.0, 1.0], [1.0, 1.0, 0.5]])
    y2[0, 1] = NAN
    ls2 = torch.tensor([-0.5, 0.2, -1.0])
    xd, ld = x2.to(DEV).requires_grad_(True), ls2.to(DEV).requires_grad_(True)
    out = S.sample_loglik(xd, N2, y2.to(DEV), m2.to(DEV), stats=True, log_std=ld)
    assert out[0].grad_fn is not None and not type(out[0].grad_fn).__name__.startswith('_SampleLoglik')
    ref = engine.sample_loglik_tensor_ops(x2.double().to(DEV), N2, y2.double().to(DEV), m2.double().to(DEV), stats=True, log_std=ls2.double().to(DEV))
    A = 0.5 * (-2.0 * ref[1]).abs() + float((m2.double() * (2.0 * ls2.double() + LOG2PI).abs()).sum(-1).max())      # >= A_n
    E = (W2 + 12) * U * A + U * LOG2PI * 3
    assert _ratio(out[1], ref[1], E) < 1.0
    assert _ratio(out[0], ref[0], E.max(1).values + U * ref[1].abs().max(1).values + _lse_slack(ref[1].max(1).values, N2, N2)) < 1.0
    gx, gl = torch.autograd.grad(out[0].sum(), (xd, ld))
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0 and float(gx[:N2, 1].abs().max()) == 0 and float(gl.abs().min()) > 0


def test_a_nan_log_std_at_an_observed_entry_stays_in_its_own_group():
    G, N, W = 3, 4, 70
    gen = torch.Generator().manual_seed(12)
    c = dict(x=torch.randn(G * N, W, generator=gen), y=torch.randn(G, W, generator=gen), m=torch.ones(G, W))
    ls = torch.zeros(G, W)
    ls[1, 69] = NAN
    clean = torch.zeros(G, W)
    outs = []
    for l in (ls, clean):
        xd, ld = c['x'].to(DEV).requires_grad_(True), l.to(DEV).requires_grad_(True)
        o = S.sample_loglik(xd, N, c['y'].to(DEV), c['m'].to(DEV), stats=True, log_std=ld)
        g = torch.autograd.grad(o[0][0] + o[0][2] + o[1][0].sum(), (xd, ld))
        outs.append((o, g))
    (o, g), (o2, g2) = outs
    assert bool(torch.isnan(o[1][1]).all()) and bool(torch.isnan(o[0][1])) and bool(torch.isfinite(o[0][[0, 2]]).all())
    assert bool(torch.isfinite(o[1][[0, 2]]).all()) and bool(torch.isfinite(o[3]).all()) and torch.equal(o[2], o2[2])
    keep = [0, 2]      # (the poisoned group's own gradients are NaN: 0 * NaN in its softmax)
    assert torch.equal(g[0].reshape(G, N, W)[keep], g2[0].reshape(G, N, W)[keep]) and torch.equal(g[1][keep], g2[1][keep])
    assert float(g[1][0].abs().min()) > 0 and bool(torch.isfinite(g[1][keep]).all())


# ---- the buffer contract of the three entry points ---------------------------------------------------------------------------------------

NAMES = ('snsde_sample_loglik_noise', 'snsde_sample_loglik_noise_backward', 'snsde_sample_loglik_noise_reduce')


@pytest.mark.parametrize('entry', [False, True], ids=['channel', 'entry'])
@pytest.mark.parametrize('shape', [(3, 5, 2, 3), (3, 2, 1, 2049), (2, 9, 3, 343), (2, 65, 3, 43), (2, 256, 5, 13), (8, 12, 2, 37)], ids=str)
def test_buffer_contract(shape, entry):
    """tests/test_gpu_buffer_contract.py's assertions on the new entry points: every output fully written whatever its memory held,
    no byte outside it written, the inputs unchanged, and the unaligned bits equal to the aligned ones (include/snsde.h promises
    it).  Finite inputs, as there."""
    G, N, O, W = shape
    norm = bool((G + N) % 2)
    gen = torch.Generator().manual_seed(G + 7 * N + 31 * O + 101 * W)
    rand = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    target = rand(O, G, W)
    ys = (target.reshape(O, G, 1, W) + 0.4 * rand(O, G, N, W)).reshape(O, G * N, W).contiguous()
    mask = (torch.rand(O, G, W, generator=gen) > 0.4).float().to(DEV)
    if G >= 2:
        mask[:, 0], mask[:, 1] = 0.0, 1.0
    ls = 0.3 * (rand(O, G, W) if entry else rand(W)) - 0.5
    lw, gl, gb = 0.5 * rand(G, N), rand(G, N), rand(G)
    before = {n: len(ALIGNMENT_SEEN.get(n, ())) for n in NAMES}

    def both():
        bound, logpx, count, sqerr = engine.sample_loglik(ys, N, target, mask, members=1, log_weight=lw, norm=norm, stats=True, log_std=ls)
        engine.sample_loglik_noise_backward(gl, gb, ys, target, mask, ls, logpx, count, N, 1, lw, norm, True, True, True)
    names = NAMES[:2] if entry else NAMES
    run_contract(f'{shape} norm={norm}', both, *names)
    if entry and shape == (8, 12, 2, 37):      # the reduce over more than one block of rows, on its own (the partial plane)
        big = rand(3, 50, W)
        run_contract(f'{shape} reduce 150 rows', lambda: engine.sample_loglik_noise_reduce(big), NAMES[2])
        names = NAMES
    if shape == (3, 5, 2, 3):      # no weights, one upstream gradient, no optional gradient
        def bare():
            bound, logpx, count, sqerr = engine.sample_loglik(ys, N, target, mask, norm=norm, stats=True, log_std=ls)
            engine.sample_loglik_noise_backward(None, gb, ys, target, mask, ls, logpx, count, N, 1, None, norm, False, False, False)
        run_contract(f'{shape} bare', bare, *NAMES[:2])
    for n in names:
        seen = ALIGNMENT_SEEN[n][before[n]:]
        assert seen and all(seen), (n, seen)


# ---- a recorded training step with the noise a live parameter ----------------------------------------------------------------------------

TIMES = np.array([0., 1., 2., 3., 4., 5.], np.float32)


def test_a_graphed_step_trains_the_model_and_the_noise_on_a_nan_marked_target():
    Sn, B, H, Cn, out_time = 4, 4, 64, 3, 2
    pr = make_problem(31, 4, 17, 2, B, H, Cn, len(TIMES), times=TIMES)
    torch.manual_seed(700)
    func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=17)
    model = train.ObservationNoise(S.NeuralSDE_forecasting(func, Cn, out_time, H, Cn), Cn, std=0.5).to(DEV).train()
    model2 = copy.deepcopy(model)
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    true = np.random.default_rng(4).standard_normal((B, out_time, Cn)).astype(np.float32)
    true[0, 1, 2] = true[2, 0, 0] = true[3, 1, 1] = np.nan
    true = torch.from_numpy(true).to(DEV)
    lengths = torch.full((B,), len(TIMES) - 1, device=DEV)
    kwargs = {'method': 'euler', 'options': {'seed': 9, 'samples': Sn, 'sample_grad': True}}
    seen = []

    def loss_of(net):
        base = S.iwae_loss(Sn, noise=net)

        def loss_fn(pred, y):
            assert tuple(pred.shape) == (B * Sn, out_time, Cn)
            loss = base(pred, y)
            seen.append(loss.detach())      # (under capture: a view of the recording's loss, refreshed by every replay)
            return loss
        return loss_fn

    start = model.log_std.detach().clone()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    eager_fn = loss_of(model)
    for _ in range(3):
        eager_fn(model(times, (coeffs,), lengths, **kwargs), true).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    eager = [t.clone() for t in seen]
    del seen[:]
    opt2 = torch.optim.Adam(model2.parameters(), lr=1e-2, capturable=True)
    graphed = train.GraphedStep(model2, times, opt2, loss_of(model2), kwargs, torch.device(DEV), warmup=1)
    graphed((coeffs,), true, lengths)      # the warm-up step of this batch shape: eager
    graphed((coeffs,), true, lengths)      # recorded, then replayed
    after_two = seen[-1].clone()
    graphed((coeffs,), true, lengths)      # replayed: reads the log_std the recorded Adam updated in place
    torch.cuda.synchronize()
    assert graphed.disabled is None and graphed.replays == 2, graphed.disabled
    assert torch.equal(seen[0], eager[0]) and torch.equal(after_two, eager[1]) and torch.equal(seen[-1], eager[2])
    assert bool(torch.isfinite(eager[2])) and not torch.equal(eager[1], eager[2])
    for (n, p), p2 in zip(model.named_parameters(), model2.parameters()):
        assert torch.equal(p, p2) and bool(torch.isfinite(p).all()), n
    assert float((model2.log_std.detach() - start).abs().min()) > 0


# ---- the differentiable filter with a learned noise --------------------------------------------------------------------------------------

def test_the_differentiable_filter_fills_the_gradient_of_a_log_std_its_likelihood_closes_over():
    """8 rows x 4 particles over 3 observations; the likelihood closes over a (W,) log_std parameter.  The same filter with
    sample_loglik_tensor_ops in the closure takes the same solves, uniforms and resampling kernel, so the two runs differ by the
    float32 round-off of the likelihood alone: logpx of the two statements lie within eps_k = E_kernel + E_ops of each other
    (module docstring: ((Dd + 11) + (V + 12)) u A_n, Dd = ceil(3 / 32) + 5 = 6, + 2 u log 2 pi count, A_n <= |logpx_n| + T), which moves a weight relatively by
    expm1(2 eps_k) - beside the resampling step's own delta_k of tests/test_gpu_filter_grad.py (profiles/filter_grad_margins.txt),
    carried on linearly as there: TOL = 2 sum_k (delta_k + expm1(2 eps_k)) of the gradient's largest entry."""
    case = STEP_OFFSET_CASES[1]
    rows, Sn, W = 8, 4, 3
    pr = make_problem(9, case.io, case.no, case.NL, rows, case.H, case.C, 7)
    m = S.Diffusion_model(case.C, case.H, case.H, case.NL, input_option=case.io, noise_option=case.no)
    with torch.no_grad():
        for name, q in m.named_parameters():
            q.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(DEV)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    y0, ts = torch.from_numpy(pr['y0']).to(DEV), torch.tensor([0.0, 1.0, 2.0, 3.0], device=DEV)
    options = {'samples': Sn, 'seed': 77, 'kernel': case.kernel}
    grads, tols, results = [], [], []
    for fn in (engine.sample_loglik, engine.sample_loglik_tensor_ops):
        log_std = torch.nn.Parameter(torch.tensor([-0.7, -0.2, -1.1], device=DEV))
        kept = []

        def likelihood(k, yk):
            obs = torch.full((yk.shape[0] // Sn, W), 0.1 * k, device=yk.device)
            logpx = fn(yk[:, :W].contiguous(), Sn, obs, log_std=log_std, stats=True)[1]
            kept.append(logpx.detach())
            return logpx
        m.zero_grad()
        r = S.sdeint_filter(m, y0, ts, likelihood, method='euler', dt=0.25, options=options, threshold=1.0,
                            generator=torch.Generator(DEV).manual_seed(5), differentiable=True)
        (-r.logz[-1].mean()).backward()
        grads.append(log_std.grad.clone())
        results.append(r)
        T = float((2.0 * log_std.detach().double() + LOG2PI).abs().sum())
        tols.append([float(((6 + 11) + (W + 12)) * U * (lp.double().abs().max() + T) + 2 * U * LOG2PI * W) for lp in kept])
    assert torch.equal(results[0].ancestor, results[1].ancestor), 'the two runs take the same ancestors'
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().min()) > 0
    lw, tol = torch.zeros(rows, Sn, device=DEV), 0.0
    for k in (1, 2, 3):      # the weights that entered each resampling step, from the run itself
        inc = engine.sample_loglik(results[0].ys[k][:, :W].detach().contiguous(), Sn, torch.full((rows, W), 0.1 * k, device=DEV),
                                   log_std=torch.tensor([-0.7, -0.2, -1.1], device=DEV), stats=True)[1]
        tol += 2 * (step_bound(lw + inc) + math.expm1(2 * max(tols[0][k - 1], tols[1][k - 1])))
        lw = results[0].log_weight[k].detach()
    diff, scale = float((grads[0] - grads[1]).abs().max()), float(grads[1].abs().max())
    _report(f'filter with a learned log_std: |kernel - tensor ops| {diff:.3e} of {scale:.3e} = {diff / scale:.3e}, TOL {tol:.3e}')
    assert 1e-7 < tol < 1e-2, tol
    assert diff <= tol * scale, (diff, tol, scale)
