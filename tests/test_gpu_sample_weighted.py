"""The weighted statistics, CRPS and quantiles of sample paths on the GPU (csrc/snsde_weighted.hip), through
sample_stats / sample_crps / sample_quantiles with log_weight=.  The float64 statement and every bound come from
tests/sample_weighted_reference.py, which derives them from the summation order documented in include/snsde.h; u = 2^-24.
Every test prints max err / bound."""
import functools
import math

import numpy as np
import pytest
import torch

from stable_neural_sdes_amd import _lib, engine
from tests import sample_weighted_reference as R
from tests.buffer_arena import FILLS, Arena, place, recorded_calls, replay, same_bits

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
U = R.U32
Q = len(R.LEVELS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, scale):
    return R.make_case(shape, scale)


def _run(x, logw, y, g, g2, gq, fair, var=True):
    """Everything the three functions give on one pooled set (G, N, W): forward and backward, as numpy float64."""
    G, N, W = x.shape
    xd, lw, yd = _dev(x).reshape(G * N, W), _dev(logw), _dev(y)
    out = {}
    xs = xd.clone().requires_grad_(True)
    mean, v = engine.sample_stats(xs, N, var=var, log_weight=lw)
    assert type(mean.grad_fn).__name__.startswith('_SampleStatsWeighted')
    loss = (mean * _dev(g)).sum() + ((v * _dev(g2)).sum() if var else 0.0)
    out['mean'], out['var'] = _np(mean), (_np(v) if var else None)
    out['stats_grad'] = _np(torch.autograd.grad(loss, xs)[0]).reshape(G, N, W)
    xc, yc = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    crps, rank, ties = engine.sample_crps(xc, N, yc, fair=fair, rank=True, log_weight=lw)
    assert type(crps.grad_fn).__name__.startswith('_SampleCRPSWeighted')
    gx, gy = torch.autograd.grad(crps, (xc, yc), _dev(g))
    out.update(crps=_np(crps), rank=_np(rank), ties=_np(ties), grad_x=_np(gx).reshape(G, N, W), grad_y=_np(gy))
    xq = xd.clone().requires_grad_(True)
    qv = engine.sample_quantiles(xq, N, R.LEVELS, log_weight=lw)
    assert type(qv.grad_fn).__name__.startswith('_SampleQuantilesWeighted')
    out['q'] = _np(qv)
    out['q_grad'] = _np(torch.autograd.grad(qv, xq, _dev(gq))[0]).reshape(G, N, W)
    return out


def _compare(got, x, logw, y, g, g2, gq, fair, var, what, chain=None):
    """`got` against the float64 statement on (x, logw, y), each quantity in units of its derived bound; returns the ratios."""
    rs = R.stats(x, logw, g, g2 if var else None, chain=chain)
    rc = R.crps(x, logw, y, fair, g, chain=chain)
    rq = R.quantiles(x, logw, R.LEVELS, gq, chain=chain)
    ratios = dict(mean=R.ratio(got['mean'], rs['mean'], rs['E_mean']), stats_grad=R.ratio(got['stats_grad'], rs['grad'], rs['E_grad']),
                  crps=R.ratio(got['crps'], rc['crps'], rc['E_crps']), rank=R.ratio(got['rank'], rc['rank'], rc['E_rank']),
                  ties=R.ratio(got['ties'], rc['ties'], rc['E_ties']), grad_x=R.ratio(got['grad_x'], rc['grad_x'], rc['E_grad_x']),
                  grad_y=R.ratio(got['grad_y'], rc['grad_y'], rc['E_grad_y']), q=R.ratio(got['q'], rq['out'], rq['E']))
    if var:
        ratios['var'] = R.ratio(got['var'], rs['var'], rs['E_var'])
    share = 1.0 - float(rq['pinned'].mean())
    cols = np.broadcast_to(rq['col_pinned'][:, None, :], got['q_grad'].shape)
    ratios['q_grad'] = R.ratio(np.where(cols, got['q_grad'], 0.0), np.where(cols, rq['grad'], 0.0), rq['E_grad'])
    print(f'{what}: err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()) + f'; brackets set aside {share:.4f}')
    assert share <= R.SHARE_CAP, (what, share)
    assert max(ratios.values()) <= 1.0, (what, ratios)
    return ratios


@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_forward_and_backward_against_float64(shape, scale):
    """All three functions, forward and backward, within the derived bounds on inputs with planted ties (sample 1 duplicates sample
    0, the observation equals sample 2); fair where N >= 2, and the non-fair score everywhere.  Quantile gradients only in columns
    whose brackets are pinned at every level; the share of unpinned (level, group, column) entries is at most SHARE_CAP.  A second
    launch gives the same bits."""
    G, N, W = shape
    c = _case(shape, scale)
    args = (c['x'], c['logw'], c['y'], c['g'], c['g2'], c['gq'])
    for fair in ([True, False] if N >= 2 else [False]):
        var = N >= 2
        got = _run(*args, fair, var)
        _compare(got, *args, fair, var, f'{shape} scale {scale} fair={fair}')
        again = _run(*args, fair, var)
        for k, v in got.items():
            assert v is None or np.array_equal(v, again[k], equal_nan=True), k
    if N > 2:
        assert (got['ties'] > 0).all()
    # no gradient asked: the plain launches give the bits of the autograd nodes
    xd, lw = _dev(c['x']).reshape(G * N, W), _dev(c['logw'])
    assert np.array_equal(_np(engine.sample_quantiles(xd, N, R.LEVELS, log_weight=lw)), got['q'], equal_nan=True)
    assert np.array_equal(_np(engine.sample_crps(xd, N, _dev(c['y']), fair=False, log_weight=lw)), got['crps'])
    assert np.array_equal(_np(engine.sample_stats(xd, N, var=False, log_weight=lw)[0]), got['mean'])


def test_pooled_members_and_a_leading_axis():
    """(outer, M, G, S, W) = (2, 3, 2, 4, 6): the members axis is addressing only - the pooled call equals the float64 statement on
    the permuted (outer G, M S, W) sets and gives the bits of the members = 1 call on that tensor."""
    O, M, G, Sn, W = R.POOLED
    N = M * Sn
    rng = np.random.default_rng(5)
    ys = rng.standard_normal((O, M, G * Sn, W)).astype(np.float32)
    logw = (2.0 * rng.standard_normal((O, G, N))).astype(np.float32)
    y, g = rng.standard_normal((O, G, W)).astype(np.float32), rng.standard_normal((O, G, W)).astype(np.float32)
    gq = rng.standard_normal((Q, O, G, W)).astype(np.float32)
    x = R.pool(ys, M, Sn)
    yd, lw = _dev(ys).requires_grad_(True), _dev(logw)
    crps, rank, ties = engine.sample_crps(yd, Sn, _dev(y), fair=True, members=M, rank=True, log_weight=lw)
    gx, = torch.autograd.grad(crps, yd, _dev(g))
    qv = engine.sample_quantiles(yd, Sn, R.LEVELS, members=M, log_weight=lw)
    gqx, = torch.autograd.grad(qv, yd, _dev(gq))
    rc = R.crps(x, logw.reshape(O * G, N), y.reshape(O * G, W), True, g.reshape(O * G, W))
    rq = R.quantiles(x, logw.reshape(O * G, N), R.LEVELS, gq.reshape(Q, O * G, W))
    ratios = dict(crps=R.ratio(_np(crps).reshape(O * G, W), rc['crps'], rc['E_crps']),
                  rank=R.ratio(_np(rank).reshape(O * G, W), rc['rank'], rc['E_rank']),
                  grad_x=R.ratio(R.pool(_np(gx), M, Sn), rc['grad_x'], rc['E_grad_x']),
                  q=R.ratio(_np(qv).reshape(Q, O * G, W), rq['out'], rq['E']))
    cols = np.broadcast_to(rq['col_pinned'][:, None, :], rq['grad'].shape)
    ratios['q_grad'] = R.ratio(np.where(cols, R.pool(_np(gqx), M, Sn), 0.0), np.where(cols, rq['grad'], 0.0), rq['E_grad'])
    print('pooled: err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0 and 1.0 - rq['pinned'].mean() <= R.SHARE_CAP
    flat = _dev(x).reshape(O * G * N, W)
    one = engine.sample_crps(flat, N, _dev(y).reshape(O * G, W), fair=True, log_weight=lw.reshape(O * G, N))
    assert torch.equal(one.reshape(O, G, W), crps.detach())
    assert torch.equal(engine.sample_quantiles(flat, N, R.LEVELS, log_weight=lw.reshape(O * G, N)).reshape(Q, O, G, W), qv.detach())


DEAD_SHAPES = [s for s in R.SHAPES if s[1] > 2]


@pytest.mark.parametrize('how', ['minus_inf', 'underflow'])
@pytest.mark.parametrize('shape', DEAD_SHAPES, ids=str)
def test_a_dead_sample_reaches_nothing(shape, how):
    """One sample of every group is dead - its weight -Inf, or mx - 200 so that expf underflows to 0 - and holds NaN in the even
    columns and +Inf in the odd ones.  Every output and every live gradient equals, within the same bounds, the float64 statement
    on the set with that sample removed; the dead sample's gradient is an exact zero."""
    G, N, W = shape
    c = _case(shape, 1.0)
    dead = N // 2 + 1 if N // 2 + 1 < N else N - 1      # (not one of the planted ties 0, 1, 2 where the set is large enough)
    x, logw = c['x'].copy(), c['logw'].copy()
    x[:, dead, 0::2] = np.nan
    x[:, dead, 1::2] = np.inf
    logw[:, dead] = -np.inf if how == 'minus_inf' else np.delete(logw, dead, 1).max(1) - np.float32(200.0)
    y = c['y'] if dead != 2 else c['x'][:, 0].copy()
    for fair in (True, False):
        got = _run(x, logw, y, c['g'], c['g2'], c['gq'], fair)
        for k in ('stats_grad', 'grad_x', 'q_grad'):
            assert (got[k][:, dead] == 0).all() and not np.signbit(got[k][:, dead]).any(), k
            got[k] = np.delete(got[k], dead, 1)
        _compare(got, np.delete(c['x'], dead, 1), np.delete(logw, dead, 1), y, c['g'], c['g2'], c['gq'], fair, True,
                 f'{shape} dead by {how} fair={fair}', chain=N)


@pytest.mark.parametrize('how', ['all_minus_inf', 'nan', 'plus_inf'])
def test_an_unusable_weight_set_is_nan_and_touches_no_other_group(how):
    """Group 1 of (3, 5, 33) has weights that are all -Inf, or one NaN, or one +Inf: NaN in every output and gradient element of
    the group; groups 0 and 2 carry the bits of a run without it."""
    shape = (3, 5, 33)
    G, N, W = shape
    c = _case(shape, 1.0)
    logw = c['logw'].copy()
    if how == 'all_minus_inf':
        logw[1] = -np.inf
    else:
        logw[1, 3] = np.nan if how == 'nan' else np.inf
    keep = [0, 2]
    sub = lambda a, axis=0: np.take(a, keep, axis)
    for fair in (True, False):
        got = _run(c['x'], logw, c['y'], c['g'], c['g2'], c['gq'], fair)
        ref = _run(sub(c['x']), sub(logw), sub(c['y']), sub(c['g']), sub(c['g2']), sub(c['gq'], 1), fair)
        for k, v in got.items():
            axis = 1 if k == 'q' else 0
            assert np.isnan(np.take(v, [1], axis)).all(), (how, fair, k)
            assert np.array_equal(sub(v, axis), ref[k]), (how, fair, k)


def _unweighted(x, y, g, g2, gq, fair):
    """The existing equal-weight kernels on a pooled set, forward and backward."""
    G, N, W = x.shape
    xd, yd = _dev(x).reshape(G * N, W), _dev(y)
    out = {}
    xs = xd.clone().requires_grad_(True)
    mean, v = engine.sample_stats(xs, N, var=N >= 2)
    out['mean'], out['var'] = _np(mean), (_np(v) if N >= 2 else None)
    loss = (mean * _dev(g)).sum() + ((v * _dev(g2)).sum() if N >= 2 else 0.0)
    out['stats_grad'] = _np(torch.autograd.grad(loss, xs)[0]).reshape(G, N, W)
    xc, yc = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    crps, rank, ties = engine.sample_crps(xc, N, yc, fair=fair, rank=True)
    gx, gy = torch.autograd.grad(crps, (xc, yc), _dev(g))
    out.update(crps=_np(crps), rank=_np(rank), ties=_np(ties), grad_x=_np(gx).reshape(G, N, W), grad_y=_np(gy))
    out['q'] = _np(engine.sample_quantiles(xd, N, R.LEVELS))
    return out


def _unweighted_bounds(x, y, g, g2, fair):
    """First-order bounds of the equal-weight kernels against float64, from their documented order (include/snsde.h).
    mean = fl(sum / S), a chain of S additions: (S + 1) u mean|x|.  var: d = fl(x - mean^) carries E_mean + u |d|, the chain of S
    fmaf(d, d, .) gives sum (2 |d| E_mean + E_mean^2 + 3 u d^2) + S u ss, one division: all over (S - 1), plus u var.  The statistics'
    gradient gm / S + c (x - mean), c = fl(fl(2 gv) / (S - 1)): 2 u |gm| / S + |c| (E_mean + 4 u |d|).  CRPS and its gradients:
    the bounds of tests/test_gpu_sample_scores.py - (2 N + 4) u (A + B'), 4 u |g| (1 / N + |c_n| / (N D)), (N + 2) u |g| - and
    3 u (|x_(k)| + |x_(k+1)|) for a quantile; the counts are exact."""
    G, N, W = x.shape
    x64, y64, g64 = x.astype(np.float64), y.astype(np.float64), g.astype(np.float64)
    mean = x64.mean(1)
    E_mean = (N + 1) * U * np.abs(x64).mean(1)
    d = x64 - mean[:, None]
    out = dict(mean=E_mean)
    if N >= 2:
        ss = (d * d).sum(1)
        sq = 2 * np.abs(d) * E_mean[:, None] + E_mean[:, None] ** 2 + 3 * U * d * d
        out['var'] = (sq.sum(1) + N * U * ss) / (N - 1) + U * ss / (N - 1)
        c = 2 * np.abs(g2.astype(np.float64)) / (N - 1)
        out['stats_grad'] = 2 * U * np.abs(g64)[:, None] / N + c[:, None] * (E_mean[:, None] + 4 * U * np.abs(d)) + np.zeros_like(d)
    else:
        out['stats_grad'] = 2 * U * np.abs(g64)[:, None] / N + np.zeros_like(d)
    dd = x64 - y64[:, None]
    cn = (x64[:, None] < x64[:, :, None]).sum(2) - (x64[:, None] > x64[:, :, None]).sum(2) if G * N * N * W < 1 << 24 else None
    if cn is None:      # (the strict counts from a sort: no (N, N) array)
        srt = np.sort(x64, 1)
        cn = np.empty_like(x64)
        for gi in range(G):
            for w in range(W):
                cn[gi, :, w] = np.searchsorted(srt[gi, :, w], x64[gi, :, w], 'left') - (N - np.searchsorted(srt[gi, :, w], x64[gi, :, w], 'right'))
    D = N - 1 if fair else N
    out['crps'] = (2 * N + 4) * U * (np.abs(dd).sum(1) / N + (np.abs(cn) * np.abs(dd)).sum(1) / (N * D))
    out['grad_x'] = 4 * U * np.abs(g64)[:, None] * (1.0 / N + np.abs(cn) / (N * D))
    out['grad_y'] = (N + 2) * U * np.abs(g64)
    srt = np.sort(x64, 1)
    ks, _ = engine.quantile_positions(R.LEVELS, N)
    out['q'] = np.stack([3 * U * (np.abs(srt[:, k]) + np.abs(srt[:, min(k + 1, N - 1)])) for k in ks])
    out['q_gap'] = np.stack([np.abs(srt[:, min(k + 1, N - 1)] - srt[:, k]) for k in ks])
    return out


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_equal_weights_agree_with_the_unweighted_kernels(shape):
    """log_weight = zeros: statistics, CRPS (with rank / N and ties / N) and the quantile levels (0, 0.1, 0.5, 0.9, 1) agree with the
    existing kernels, forward and backward, within the sum of the two kernels' derived bounds.  The two float64 statements of a
    quantile differ by the rounding of the level itself (the weighted call takes float32(q), the unweighted one float32 of the
    fraction of q (N - 1)): at most 2 u (N - 1) of the bracket's gap, which joins the margin."""
    G, N, W = shape
    c = _case(shape, 1.0)
    zeros = np.zeros((G, N), np.float32)
    for fair in ([True, False] if N >= 2 else [False]):
        got = _run(c['x'], zeros, c['y'], c['g'], c['g2'], c['gq'], fair, N >= 2)
        old = _unweighted(c['x'], c['y'], c['g'], c['g2'], c['gq'], fair)
        eo = _unweighted_bounds(c['x'], c['y'], c['g'], c['g2'], fair)
        rs = R.stats(c['x'], zeros, c['g'], c['g2'] if N >= 2 else None)
        rc = R.crps(c['x'], zeros, c['y'], fair, c['g'])
        rq = R.quantiles(c['x'], zeros, R.LEVELS)
        ew = dict(mean=rs['E_mean'], var=rs['E_var'], stats_grad=rs['E_grad'], crps=rc['E_crps'], grad_x=rc['E_grad_x'],
                  grad_y=rc['E_grad_y'], q=rq['E'] + 2 * U * (N - 1) * eo['q_gap'])
        ratios = {}
        for k in ew:
            if old[k] is not None:
                ratios[k] = float((np.abs(got[k] - old[k]) / (ew[k] + eo[k] + R.TINY)).max())
        ratios['rank'] = float((np.abs(got['rank'] - old['rank'] / N) / (rc['E_rank'] + U * old['rank'] / N + R.TINY)).max())
        ratios['ties'] = float((np.abs(got['ties'] - old['ties'] / N) / (rc['E_ties'] + U * old['ties'] / N + R.TINY)).max())
        print(f'{shape} equal weights fair={fair}: difference / margin ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
        assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_integer_weights_agree_with_the_unweighted_kernels_on_the_replicated_set(shape):
    """log_weight = log k_n, k_n = 1 + n mod 4 (all ones where their sum would pass 256): the weighted mean, the non-fair CRPS and
    rank and ties times sum k equal the unweighted kernels on the set with sample n repeated k_n times, within the sum of the two
    bounds.  float32(log k) moves a_n by at most u log 4, so every w_n by at most 2 u log 4 relative, and the mean (linear in w) and
    the score (quadratic) by at most 6 u log 4 of their scales sum w |x| and A + B': that joins the margin."""
    G, N, W = shape
    c = _case(shape, 1.0)
    k = 1 + np.arange(N) % 4
    if k.sum() > 256:
        k = np.ones(N, np.int64)
    K = int(k.sum())
    logw = np.broadcast_to(np.log(k).astype(np.float32), (G, N)).copy()
    got = _run(c['x'], logw, c['y'], c['g'], c['g2'], c['gq'], False, N >= 2)
    rep = np.repeat(c['x'], k, axis=1)
    old = _unweighted(rep, c['y'], c['g'], c['g2'], c['gq'], False)
    eo = _unweighted_bounds(rep, c['y'], c['g'], c['g2'], False)
    rs, rc = R.stats(c['x'], logw), R.crps(c['x'], logw, c['y'], False)
    x64 = np.abs(rep.astype(np.float64))
    inp = 6 * U * math.log(4.0)
    ratios = dict(mean=(np.abs(got['mean'] - old['mean']) / (rs['E_mean'] + eo['mean'] + inp * x64.mean(1))).max(),
                  crps=(np.abs(got['crps'] - old['crps']) / (rc['E_crps'] + eo['crps'] * (1 + inp / U / (2 * K + 4)))).max(),
                  rank=(np.abs(got['rank'] * K - old['rank']) / (K * rc['E_rank'] + (inp + U) * old['rank'] + R.TINY)).max(),
                  ties=(np.abs(got['ties'] * K - old['ties']) / (K * rc['E_ties'] + (inp + U) * old['ties'] + R.TINY)).max())
    print(f'{shape} replication (sum k = {K}): difference / margin ' + ', '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


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


@pytest.mark.parametrize('optional', [True, False], ids=['all outputs', 'required only'])
@pytest.mark.parametrize('shape', [(3, 5, 33), (2, 64, 130)], ids=str)
def test_buffer_contract_of_the_six_entry_points(shape, optional):
    G, N, W = shape
    c = _case(shape, 1.0)
    ys, lw, y = _dev(c['x']).reshape(G * N, W), _dev(c['logw']), _dev(c['y'])
    g, g2, gq = _dev(c['g']), _dev(c['g2']), _dev(c['gq'])

    def thunk():
        mean, _ = engine.sample_stats(ys, N, var=optional, log_weight=lw)
        engine.sample_stats_weighted_backward(g, g2 if optional else None, ys, lw, mean, N)
        engine.sample_crps(ys, N, y, fair=optional, rank=optional, log_weight=lw)
        engine.sample_crps_weighted_backward(g, ys, y, lw, N, fair=optional, grad_target=optional)
        engine.sample_quantiles(ys, N, R.LEVELS if optional else [0.3], log_weight=lw)
        engine.sample_quantiles_weighted_backward(gq if optional else gq[:1].contiguous(), ys, lw, N, R.LEVELS if optional else [0.3])
    with recorded_calls(engine) as rec:
        thunk()
    torch.cuda.current_stream().synchronize()
    for name in ('snsde_sample_stats_weighted', 'snsde_sample_crps_weighted', 'snsde_sample_quantiles_weighted'):
        _hold(rec.named(name), f'{shape}')
        _hold(rec.named(name + '_backward'), f'{shape}')


def test_forward_and_backward_replay_from_one_graph():
    """One capture of forward + backward of the weighted CRPS; its replay gives the eager bits."""
    shape = (3, 5, 33)
    G, N, W = shape
    c = _case(shape, 4.0)
    xd, lw, yd, g = _dev(c['x']).reshape(G * N, W).requires_grad_(True), _dev(c['logw']), _dev(c['y']).requires_grad_(True), _dev(c['g'])

    def step():
        crps = engine.sample_crps(xd, N, yd, log_weight=lw)
        gx, gy = torch.autograd.grad(crps, (xd, yd), g)
        return crps.detach(), gx, gy

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()      # (warm-up outside the capture, on a side stream as capture asks)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    with torch.no_grad():
        for t in static:
            t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(('crps', 'grad_ys', 'grad_target'), static, eager):
        assert torch.equal(a, b), name


def test_filter_recipe_on_the_gpu():
    """sample_stats(filter_particles(ys, ancestor, S), S, log_weight=) of a hand-made filter result equals the float64 statement on
    the hand-gathered sets, all times in one launch."""
    T, B, Sn, H = 3, 4, 8, 5
    rng = np.random.default_rng(11)
    ys = rng.standard_normal((T, B * Sn, H)).astype(np.float32)
    anc = rng.integers(0, Sn, (T, B, Sn)).astype(np.int32)
    logw = rng.standard_normal((T, B, Sn)).astype(np.float32)
    mean, var = engine.sample_stats(engine.filter_particles(_dev(ys), _dev(anc), Sn), Sn, log_weight=_dev(logw))
    hand = np.take_along_axis(ys.reshape(T * B, Sn, H), anc.reshape(T * B, Sn, 1).astype(np.int64), 1)
    r = R.stats(hand, logw.reshape(T * B, Sn))
    rm, rv = R.ratio(_np(mean).reshape(T * B, H), r['mean'], r['E_mean']), R.ratio(_np(var).reshape(T * B, H), r['var'], r['E_var'])
    print(f'filter recipe: err / bound mean {rm:.3f}, var {rv:.3f}')
    assert rm <= 1.0 and rv <= 1.0
