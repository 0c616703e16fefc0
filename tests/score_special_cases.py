"""Special sample sets - NaN, +-Inf, signed zeros, all-equal sets, duplicated extremes - for the statistics and score kernels
(sample_stats, ensemble_stats, sample_crps, sample_quantiles, sample_energy), and float64 numpy references with IEEE semantics.
Plain data, importable without a GPU; tests/test_score_specials_cpu.py checks the references and the fixture's premises,
tests/test_gpu_score_specials.py holds the kernels to them.

The inputs.  `build(shape, layout)` gives a clean seeded randn tensor x (G, N, W) and an observation y (G, W), finite magnitudes
<= 8, with one pattern of PATTERNS planted per slot: a slot is a column (g, w) - or, for the energy score whose sample is a
vector, a group g (`vector=True`).  The slots of a shape are every second column (every second group), so each special set has
clean neighbours, and the shape's `layouts(shape)` together plant every pattern at least once.  A shape with more than 8 groups
(the grid-stride shape) has its slots in groups 5 and 6 only.  `special=False` gives the same tensors with nothing planted: the
two differ in the slots alone.

The contract (the references below state it in numpy).  Forward: the documented formula in float64 on the float32 inputs, counts
from O(N^2) IEEE comparisons (a NaN compares false both ways), signs from np.sign; every output element has a class - finite,
+Inf, -Inf, NaN - that the code under test must reproduce, and where it is finite the existing error bound of that function
applies.  With finite magnitudes <= 8 nothing finite overflows in float32, so the class does not depend on the summation order.
Quantiles: a set that holds a NaN gives NaN at every level (torch.quantile's rule); a set with +-Inf and no NaN follows the
formula (x_(k), or x_(k) + frac (x_(k+1) - x_(k)) where frac != 0: interpolating from -Inf or between equal infinities is NaN).
Backward: prescribed only where the forward value of the set is finite: the documented formula with sign(0) = 0 and
d||d|| = 0 at d = 0."""
import functools

import numpy as np

U = 2.0 ** -24
QS = (0.0, 0.1, 0.5, 0.9, 1.0)
PATTERNS = ('nan_first', 'nan_last', 'pos_inf', 'neg_inf', 'both_inf', 'two_pos_inf', 'all_nan', 'all_equal', 'all_equal_obs',
            'signed_zeros', 'dup_extremes', 'obs_nan', 'obs_inf')
CLEAN = -1      # pattern index of a set nothing was planted in
SHAPES = [(1, 2, 3), (2, 5, 70), (2, 17, 5), (1, 256, 4), (8200, 3, 2)]      # (G, N, W)
ENERGY_SHAPES = SHAPES + [(2, 5, 17)]                                         # one column past a chunk of 16
ENSEMBLE = (2, 3, 2, 4, 6)                                                    # (outer, M, G, S, W)
BIG_GROUPS = (5, 6)                                                           # the slots of a shape with more than 8 groups
# The shape tables of the float64 GPU tests of the same kernels, moved here unchanged so that other tests can share them; each test
# module says why its shapes are there.
SCORE_SHAPES = [(1, 2, 1), (3, 5, 33), (2, 64, 130), (1, 256, 4), (9000, 3, 2)]      # tests/test_gpu_sample_scores.py: (G, N, W)
ENSEMBLE_STATS_SHAPES = [(2, 3, 5, 4, 64), (1, 2, 3, 2, 7), (1, 4, 1, 3, 1)]         # tests/test_gpu_ensemble_stats.py: (outer, M, G, S, W)
LOGLIK_SHAPES = [(1, 1, 1, 1), (3, 5, 2, 3), (2, 8, 1, 64), (2, 8, 1, 65), (2, 7, 3, 130), (1, 256, 1, 4), (9000, 2, 1, 2),
                 (2, 8, 1, 2048), (1, 2, 1, 2049), (1, 9, 1, 1025), (2, 16, 2, 40), (2, 17, 1, 70), (2, 32, 1, 513), (2, 33, 1, 257),
                 (2, 64, 1, 256), (2, 65, 1, 129), (1, 128, 1, 128), (1, 129, 1, 65)]  # tests/test_gpu_sample_loglik.py: (G, N, outer, W)
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3


def slots(shape, vector=False):
    """The sets a pattern may be planted in: [(g, w), ..] or, vector=True, [g, ..]."""
    G, N, W = shape
    if vector:
        return list(BIG_GROUPS) if G > 8 else list(range(0, G, 2))
    if G > 8:
        return [(g, w) for g in BIG_GROUPS for w in range(W)]
    return [(g, w) for g in range(G) for w in range(W) if (g * W + w) % 2 == 0]


def layouts(shape, vector=False):
    """How many layouts plant every pattern at least once."""
    n = len(slots(shape, vector))
    return (len(PATTERNS) + n - 1) // n


def special_component(W):
    """The component of a vector sample a non-finite value is planted in: 16 (one past a chunk) where there is one, else the last."""
    return 16 if W > 16 else W - 1


def _plant(name, col, ycol, span):
    """Plant pattern `name` in the sample set col (N,) (a view) and its observation ycol (a 0-d view); the single special samples
    go to the first / middle / last index of span = (n_lo, n_hi)."""
    N = col.shape[0]
    first, last, mid = span[0], span[1] - 1, (span[0] + span[1]) // 2
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    if name == 'nan_first':
        col[first] = nan
    elif name == 'nan_last':      # the minimum at sample 0: another wave's quarter than the NaN
        col[0] = np.float32(col[:last].min() - 0.5) if last > 0 else col[0]
        col[last] = nan
    elif name == 'pos_inf':
        col[mid] = inf
    elif name == 'neg_inf':
        col[mid] = -inf
    elif name == 'both_inf':
        col[first], col[last] = inf, -inf
    elif name == 'two_pos_inf':
        col[first] = col[last] = inf
    elif name == 'all_nan':
        col[:] = nan
    elif name == 'all_equal':
        col[:] = col[0]
    elif name == 'all_equal_obs':
        col[:] = col[0]
        ycol[...] = col[0]
    elif name == 'signed_zeros':
        col[0::2], col[1::2] = np.float32(0.0), np.float32(-0.0)
        ycol[...] = np.float32(-0.0)
    elif name == 'dup_extremes':      # the minimum at both ends, the maximum next to them: duplicates in different quarters
        lo, hi = np.float32(col.min() - 0.5), np.float32(col.max() + 0.5)
        col[0] = col[N - 1] = lo
        if N >= 3:
            col[1] = hi
        if N >= 4:
            col[N - 2] = hi
    elif name == 'obs_nan':
        ycol[...] = nan
    elif name == 'obs_inf':
        ycol[...] = inf
    else:
        raise KeyError(name)


@functools.lru_cache(maxsize=None)
def build(shape, layout=0, vector=False, special=True, span=None):
    """x (G, N, W), y (G, W) float32 and the pattern index of every set ((G, W), or (G,) for vector=True; CLEAN where nothing
    is planted).  Read-only: shared by every test that asks for the same arguments."""
    G, N, W = shape
    rng = np.random.default_rng(1000 * N + W)
    x = np.clip(2.0 * rng.standard_normal((G, N, W)) + 0.5, -7.0, 7.0).astype(np.float32)
    y = np.clip(rng.standard_normal((G, W)), -7.0, 7.0).astype(np.float32)
    sl = slots(shape, vector)
    pat = np.full((G,) if vector else (G, W), CLEAN, np.int64)
    span = span or (0, N)
    for i, s in enumerate(sl):
        p = (layout * len(sl) + i) % len(PATTERNS)
        pat[s] = p
        if not special:
            continue
        name = PATTERNS[p]
        if not vector:
            _plant(name, x[s[0], :, s[1]], y[s[0], s[1]:s[1] + 1].reshape(()), span)
        elif name in ('all_equal', 'all_equal_obs', 'signed_zeros', 'dup_extremes'):      # whole vectors
            for w in range(W):
                _plant(name, x[s, :, w], y[s, w:w + 1].reshape(()), span)
        else:
            v = special_component(W)
            _plant(name, x[s, :, v], y[s, v:v + 1].reshape(()), span)
    assert float(np.abs(x[np.isfinite(x)]).max()) <= 8.0 and float(np.abs(y[np.isfinite(y)]).max()) <= 8.0
    for a in (x, y, pat):
        a.setflags(write=False)
    return x, y, pat


def upstream(shape, n, vector=False, seed=7):
    """n finite upstream gradients (G, W) (or (G,) for vector=True), float32, fixed per shape."""
    G, N, W = shape
    rng = np.random.default_rng(seed + 10 * N + W)
    return [rng.standard_normal((G,) if vector else (G, W)).astype(np.float32) for _ in range(n)]


def classes(a):
    """FINITE / POS_INF / NEG_INF / NAN of every element."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), NAN, np.where(a == np.inf, POS_INF, np.where(a == -np.inf, NEG_INF, FINITE)))


def to_members(x, outer, M, S):
    """Pooled sets (outer G, N = M S, W), n = m S + s  ->  the ensemble layout (outer, M, G, S, W)."""
    OG, N, W = x.shape
    return np.ascontiguousarray(x.reshape(outer, OG // outer, M, S, W).transpose(0, 2, 1, 3, 4))


# ---- float64 references ----------------------------------------------------------------------------------------------------------

def ref_sample_stats(x, gm=None, gv=None):
    """mean = sum x / S, var = sum (x - mean)^2 / (S - 1) over axis 1 of x (G, S, W); e_m, bound_v: the error bounds of
    tests/test_gpu_samples.py::test_sample_stats_against_float64; gx: grad_mean / S + grad_var 2 (x - mean) / (S - 1)."""
    x64 = x.astype(np.float64)
    S = x.shape[1]
    with np.errstate(all='ignore'):
        mean = x64.sum(1) / S
        var = ((x64 - mean[:, None]) ** 2).sum(1) / (S - 1) if S > 1 else None
        e_m = (S + 1) * U * np.abs(x64).sum(1) / S
        out = dict(mean=mean, var=var, e_m=e_m)
        if S > 1:
            out['bound_v'] = (S + 4) * U * var + (1 + (S + 4) * U) * S * e_m ** 2 / (S - 1)
        if gm is not None:
            g1, g2 = gm.astype(np.float64)[:, None], gv.astype(np.float64)[:, None]
            out['gx'] = g1 / S + g2 * 2 * (x64 - mean[:, None]) / (S - 1)
            # (tests/test_gpu_sample_grad.py: test_sample_stats_backward_against_float64_autograd)
            ymax = np.abs(x64).max(1)
            out['gx_bound'] = np.broadcast_to((2.0 ** -19 * (np.abs(g1[:, 0]) / S + 4 * np.abs(g2[:, 0]) * ymax / (S - 1))
                                               + 2 * np.abs(g2[:, 0]) / (S - 1) * S * U * ymax)[:, None], x64.shape)
    return out


def ref_ensemble_stats(x5, gm=None, gw=None, gb=None):
    """x5 (outer, M, G, S, W): mean of the member means, within = mean of the member variances, between = unbiased variance of
    the member means.  Bounds: e_mu and the between bound as tests/test_gpu_ensemble_stats.py derives them; within: each member
    variance within bound_v (above), M non-negative terms added in order and one division, a relative (M + 1) u on their sum."""
    x64 = x5.astype(np.float64)
    O, M, G, S, W = x5.shape
    with np.errstate(all='ignore'):
        mm = x64.sum(3) / S
        vm = ((x64 - mm[:, :, :, None]) ** 2).sum(3) / (S - 1)
        mu = mm.sum(1) / M
        within = vm.sum(1) / M
        a = mm - mu[:, None]
        between = (a ** 2).sum(1) / (M - 1)
        e_m = (S + 1) * U * np.abs(x64).sum(3) / S
        e_mu = (M + 1) * U * (np.abs(mm) + e_m).sum(1) / M + e_m.sum(1) / M
        bv = (S + 4) * U * vm + (1 + (S + 4) * U) * S * e_m ** 2 / (S - 1)
        Dm = e_m + e_mu[:, None]
        Dm = Dm + U * (np.abs(a) + Dm)
        T, R = (a ** 2).sum(1), (2 * np.abs(a) * Dm + Dm ** 2).sum(1)
        out = dict(mean=mu, within=within, between=between, e_mu=e_mu,
                   bound_w=bv.sum(1) / M + (M + 1) * U * (vm + bv).sum(1) / M,
                   bound_b=((M + 4) * U * (T + R) + R) / (M - 1))
        if gm is not None:
            A = gm.astype(np.float64)[:, None, :, None, :] / (M * S)
            Cw = 2 * gw.astype(np.float64)[:, None, :, None, :] / ((S - 1) * M)
            Cb = 2 * gb.astype(np.float64)[:, None, :, None, :] / ((M - 1) * S)
            dx, am = x64 - mm[:, :, :, None], a[:, :, :, None]
            out['gx'] = A + Cw * dx + Cb * am
            em, emu = e_m[:, :, :, None], e_mu[:, None, :, None, :]
            mag = np.abs(A) + np.abs(Cw * dx) + np.abs(Cb * am)      # (tests/test_gpu_ensemble_stats.py: test_backward_against_float64_autograd)
            out['gx_bound'] = 8 * U * mag + (1 + 8 * U) * (np.abs(Cw) * em + np.abs(Cb) * (em + emu)) + 1e-12 * mag
    return out


def _counts(x64):
    """lt[g, n, w] = #{j : x_j < x_n}, gt = #{j : x_j > x_n}, eq_before = #{j < n : x_j == x_n}: IEEE comparisons, no sort."""
    xn, xj = x64[:, :, None, :], x64[:, None, :, :]
    N = x64.shape[1]
    before = (np.arange(N)[None, :] < np.arange(N)[:, None])[None, :, :, None]      # [n, j]: j < n
    with np.errstate(invalid='ignore'):
        return (xj < xn).sum(2), (xj > xn).sum(2), ((xj == xn) & before).sum(2)


def ref_crps(x, y, fair, g=None):
    """crps = sum |d_n| / N - sum c_n d_n / (N D), rank = #{x_n < y}, ties = #{x_n == y}; scale = A + B' of the bound
    (2 N + 4) u (A + B'); gx = g (sign(d_n) / N - c_n / (N D)), gy = -g sum sign(d_n) / N with their scales
    (tests/test_gpu_sample_scores.py)."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    N = x.shape[1]
    D = N - 1 if fair else N
    lt, gt, _ = _counts(x64)
    c = (lt - gt).astype(np.float64)
    with np.errstate(all='ignore'):
        d = x64 - y64[:, None]
        out = dict(crps=np.abs(d).sum(1) / N - (c * d).sum(1) / (N * D), rank=(d < 0).sum(1), ties=(d == 0).sum(1),
                   scale=np.abs(d).sum(1) / N + (np.abs(c) * np.abs(d)).sum(1) / (N * D))
        if g is not None:
            g64 = g.astype(np.float64)
            out.update(gx=g64[:, None] * (np.sign(d) / N - c / (N * D)), gx_scale=np.abs(g64)[:, None] * (1.0 / N + np.abs(c) / (N * D)),
                       gy=-g64 * np.sign(d).sum(1) / N, gy_bound=(N + 2) * U * np.abs(g64))
    return out


def quantile_positions(q, N):
    """pos = q (N - 1) in float64, k = floor(pos), frac = float32(pos - k) (the rule engine.quantile_positions documents)."""
    ks, fracs = [], []
    for v in q:
        pos = float(v) * (N - 1)
        k = int(np.floor(pos))
        frac = float(np.float32(pos - k))
        if frac >= 1.0:
            k, frac = k + 1, 0.0
        ks.append(k)
        fracs.append(frac)
    return ks, fracs


def ref_quantiles(x, q=QS):
    """out[q] = x_(k), or x_(k) + frac (x_(k+1) - x_(k)) where frac != 0, the order statistics from permutation ranks
    rank_n = #{x_j < x_n} + #{j < n : x_j == x_n}; NaN at every level of a set that holds a NaN.  scale = |x_(k)| + |x_(k+1)| of
    the bound 3 u scale; rank (G, N, W) for the backward (meaningful where the set holds no NaN)."""
    x64 = x.astype(np.float64)
    G, N, W = x.shape
    ks, fracs = quantile_positions(q, N)
    lt, _, eqb = _counts(x64)
    rank = lt + eqb
    bad = np.isnan(x64).any(1)
    srt = np.full((G, N, W), np.nan)
    clean_rank = np.where(bad[:, None], np.arange(N)[None, :, None], rank)      # (a permutation in every column)
    np.put_along_axis(srt, clean_rank, x64, axis=1)
    out, scale = np.empty((len(ks), G, W)), np.empty((len(ks), G, W))
    with np.errstate(all='ignore'):
        for i, (k, f) in enumerate(zip(ks, fracs)):
            lo, hi = srt[:, k], srt[:, min(k + 1, N - 1)]
            out[i] = np.where(bad, np.nan, lo if f == 0.0 else lo + f * (hi - lo))
            scale[i] = np.abs(lo) + (np.abs(hi) if f != 0.0 else 0.0)
    return dict(out=out, scale=scale, rank=rank, bad=bad, ks=ks, fracs=fracs)


def ref_quantiles_grad(ref, g):
    """grad_ys[n] = sum_q g_q (1 - frac_q) [rank_n == k_q] + g_q frac_q [rank_n == k_q + 1] in float64, g (Q, G, W); and `mag`,
    the same sum over |terms| (each term is one float32 product, the sum over q adds at most 2 Q of them)."""
    rank = ref['rank']
    gx, mag = np.zeros(rank.shape), np.zeros(rank.shape)
    for i, (k, f) in enumerate(zip(ref['ks'], ref['fracs'])):
        gi = g[i].astype(np.float64)[:, None]
        f32 = float(np.float32(f))
        lo = (rank == k) * gi * (1.0 - f32)
        hi = (rank == k + 1) * gi * f32 if f != 0.0 else 0.0
        gx += lo + hi
        mag += np.abs(lo) + np.abs(hi)
    return gx, mag


def ref_energy(x, y, fair, g=None):
    """energy = sum_n ||x_n - y|| / N - sum_{n<j} ||x_n - x_j|| / (N D) per group of x (G, N, V), y (G, V); scale = A + B of the
    bound (V / 2 + 2 N + 8) u (A + B); gx, gy with d||d|| = d / ||d||, 0 at d = 0, and their bounds
    (tests/test_gpu_sample_energy.py)."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    G, N, V = x.shape
    D = N - 1 if fair else N
    iu = np.triu(np.ones((N, N), bool), 1)
    with np.errstate(all='ignore'):
        d = x64 - y64[:, None]
        rn = np.sqrt((d * d).sum(-1))
        diff = x64[:, :, None] - x64[:, None, :]
        rnj = np.sqrt((diff * diff).sum(-1))
        A = rn.sum(1) / N
        B = np.where(iu[None], rnj, 0.0).sum((1, 2)) / (N * D) if N > 1 else np.zeros(G)      # (only the pairs n < j enter)
        out = dict(energy=A - B, scale=A + B)
        if g is not None:
            g64 = g.astype(np.float64)
            un = np.where(rn[..., None] > 0, d / rn[..., None], 0.0)
            unj = np.where(rnj[..., None] > 0, diff / rnj[..., None], 0.0)
            out.update(gx=g64[:, None, None] * (un / N - (unj.sum(2) / (N * D) if N > 1 else 0.0)), gy=-g64[:, None] * un.sum(1) / N,
                       gx_bound=(V / 2 + N + 8) * U * (np.abs(g64) * (1.0 / N + (N - 1) / (N * D)))[:, None, None] * np.ones((1, N, V)),
                       gy_bound=(V / 2 + N + 8) * U * np.abs(g64)[:, None] * np.ones((1, V)))
    return out
