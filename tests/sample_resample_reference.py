"""Float64 numpy statement of the resampling step (include/snsde.h: snsde_sample_resample), with the margins of its comparisons
and the round-off bounds of the kernel's documented summation order.  Plain helpers, importable without a GPU.

Definitions, per group, n and j in 0 .. S-1:  a_n = logw_n + loginc_n (in the dtype of the inputs: float32 inputs give the
kernel's one rounded addition exactly, so a is no source of difference), mx = max a, e_n = exp(a_n - mx), P_n = e_0 + .. + e_n,
logz = mx + log P_{S-1} - log S, ess = P_{S-1}^2 / sum e_n^2, t_j = ((j + u_j) / S) P_{S-1}, ancestor[j] = #{n < S-1 : P_n <= t_j}.

Bounds (first order in the unit round-off `unit`, times 1.01 for the higher orders; x_n = mx - a_n >= 0).  The kernel computes
  e_n    = expf(fl(a_n - mx)): the rounded difference moves the exponent by x_n unit, expf is within 3 ulp = 6 unit (the OpenCL
           bound the device library documents), so |e^_n - e_n| <= e_n (x_n + 6) unit;
  P_n    by one sequential chain: addition k rounds a partial sum of size P_k, so |P^_n - P_n| <= unit (sum_{k<=n} P_k +
           sum_{k<=n} e_k (x_k + 6)) <= BP := the same with n = S - 1;
  t_j    = fl(fl(fl(j + u_j) / S) P^_{S-1}): three roundings and the error of P^_{S-1}, |t^_j - t_j| <= 3 unit t_j + BP.
A comparison P_n <= t_j can therefore only come out differently where |t_j - P_n| / P_{S-1} <= delta := 2 BP / P_{S-1} + 3 unit.
For uniform weights delta is about (S + 15) unit; weights concentrated on a few particles make it smaller.
  logz   = fl(fl(mx + logf(P^)) - logf(S)), logf within 3 ulp: E_logz = BP / P + unit (6 |log P| + 6 log S + |mx + log P| + |logz|);
  ess    = fl(fl(P^ P^) / q^), q by a chain of fmaf(e, e, q): relative 2 BP / P + 2 unit + unit (2 sum e_k^2 (x_k + 6) + sum_k q_k) / q.
logw_out is a (exact) or logz (E_logz)."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
INF = float('inf')

# (G, S, W) of the kernel tests: one element; a pack with a ragged tail; odd sizes; a wide vector row; S at the cap on a narrow
# row; odd S just below it on an odd row wider than a workgroup; many small groups
SHAPES = [(1, 1, 1), (3, 2, 5), (5, 7, 33), (2, 64, 128), (4, 256, 4), (2, 255, 257), (9001, 4, 3)]
# 64 groups of (4, 3) share a workgroup and the grid stops at 2048 workgroups: this one takes more than one grid pass
STRIDE_SHAPE = (140001, 4, 3)
THRESHOLDS = (0.0, 0.5, 1.0)
SCALES = (1.0, 4.0)                   # log-weights ~ N(0, 1) and N(0, 16)
SHARE_CAP = 0.02                      # of the (g, j) of a shape whose ancestor cannot be pinned


def make_case(shape, scale, seed=0):
    """Seeded float32 inputs of a shape: state, logw ~ N(0, scale^2), loginc ~ N(0, 1), u (G) and us (G, S) in [0, 1)."""
    G, S, W = shape
    rng = np.random.default_rng(1000003 * seed + 7919 * G + 31 * S + W + int(100 * scale))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(state=f(G, S, W), logw=(scale * f(G, S)).astype(np.float32), loginc=f(G, S),
                u=rng.random(G, dtype=np.float32), us=rng.random((G, S), dtype=np.float32))


def reference(logw, loginc, u, threshold, stratified, unit=U32):
    """logw, loginc (None: 0) of shape (G, S), u (G) or, stratified, (G, S).  Returns a dict: a, ancestor (G, S), ess, logz,
    resampled (G), logw_out (G, S), e (G, S), margin (G, S) = min_{n < S-1} |t_j - P_n| / P_{S-1} (inf for S = 1), and the bounds
    delta, E_logz, E_ess (G)."""
    a = np.asarray(logw) if loginc is None else np.asarray(logw) + np.asarray(loginc)      # (float32 inputs: one float32 rounding)
    a64 = a.astype(np.float64)
    G, S = a64.shape
    with np.errstate(all='ignore'):
        bad = np.isnan(a64).any(1) | (a64 == INF).any(1)
        mx = np.max(np.where(np.isnan(a64), -INF, a64), axis=1)
        dead = ~bad & (mx == -INF)
        kept = bad | dead
        shift = np.where(kept, 0.0, mx)
        x = np.where(kept[:, None], 0.0, shift[:, None] - a64)           # >= 0; +inf for a dead particle
        e = np.exp(-x)
        P = np.cumsum(e, axis=1)
        tot = P[:, -1]
        q = (e * e).sum(1)
        logz = np.where(bad, np.nan, np.where(dead, -INF, shift + np.log(tot) - np.log(S)))
        ess = np.where(bad, np.nan, np.where(dead, 0.0, tot * tot / q))
        always, some = threshold >= 1, threshold > 0
        res = ~kept & (np.full(G, always) | (some & (ess < threshold * S)))
        j = np.arange(S)
        uu = np.asarray(u, np.float64).reshape(G, S if stratified else 1)
        t = ((j + uu) / S) * tot[:, None]
        count = (P[:, None, :S - 1] <= t[:, :, None]).sum(-1)
        alive = e > 0
        first = alive.argmax(1)[:, None]
        last = (S - 1 - alive[:, ::-1].argmax(1))[:, None]
        anc = np.where(res[:, None], np.clip(count, first, last), j[None, :])
        margin = (np.abs(t[:, :, None] - P[:, None, :S - 1]).min(-1) / tot[:, None]) if S > 1 else np.full((G, S), INF)
        xe = np.where(alive, e * (np.where(alive, x, 0.0) + 6.0), 0.0)
        BP = unit * (P.sum(1) + xe.sum(1))
        delta = 1.01 * (2.0 * BP / tot + 3.0 * unit)
        lt = np.log(tot)
        E_logz = 1.01 * (BP / tot + unit * (6.0 * np.abs(lt) + 6.0 * np.log(S) + np.abs(shift + lt) + np.abs(np.where(kept, 0.0, logz)))) + 1e-300
        Q = np.cumsum(e * e, axis=1)
        E_ess = np.where(kept, 0.0, ess) * 1.01 * (2.0 * BP / tot + 2.0 * unit + unit * (2.0 * (e * xe).sum(1) + Q.sum(1)) / q) + 1e-300
        logw_out = np.where(res[:, None], logz[:, None], a64)
    return dict(a=a, ancestor=anc.astype(np.int64), ess=ess, logz=logz, resampled=res.astype(np.int64), logw_out=logw_out, e=e,
                margin=margin, delta=delta, E_logz=E_logz, E_ess=E_ess)


def unpinned_share(ref):
    """The share of the (g, j) of resampled groups whose comparison margin is within delta (their ancestor cannot be pinned)."""
    rows = ref['resampled'].astype(bool)
    if not rows.any():
        return 0.0
    return float((ref['margin'][rows] <= ref['delta'][rows][:, None]).mean())


def check_outputs(ref, got, threshold, S, what=''):
    """The kernel's (or the statement's) outputs against the reference with the bounds above.  got: dict of numpy arrays ancestor,
    ess, logz, resampled, logw_out.  Returns the number of (g, j) inside the margin whose ancestor differed (by one)."""
    nan = np.isnan(ref['logz'])
    assert np.array_equal(np.isnan(got['logz']), nan) and np.array_equal(np.isnan(got['ess']), nan), what
    fin = np.isfinite(ref['logz'])
    assert np.array_equal(got['logz'][~fin & ~nan], ref['logz'][~fin & ~nan]) and np.array_equal(got['ess'][~fin & ~nan], ref['ess'][~fin & ~nan]), what
    el = np.abs(got['logz'][fin] - ref['logz'][fin]) / ref['E_logz'][fin]
    ee = np.abs(got['ess'][fin] - ref['ess'][fin]) / ref['E_ess'][fin]
    assert el.size == 0 or (el.max() <= 1.0 and ee.max() <= 1.0), (what, 'logz, ess in units of their bounds', el.max(), ee.max())
    # the decision, wherever ess is not within its bound of threshold S (threshold S itself is rounded once by the kernel)
    clear = ~fin | (np.abs(ref['ess'] - threshold * S) > ref['E_ess'] + U32 * abs(threshold) * S) | (threshold <= 0) | (threshold >= 1)
    assert np.array_equal(got['resampled'][clear], ref['resampled'][clear]), what
    assert set(np.unique(got['resampled'])) <= {0, 1}, what
    same = got['resampled'] == ref['resampled']
    res = got['resampled'].astype(bool)
    # the weights: a exactly where the group is kept, logz where it is resampled
    assert np.array_equal(got['logw_out'][~res], ref['a'].astype(got['logw_out'].dtype)[~res], equal_nan=True), what
    assert np.array_equal(got['logw_out'][res], np.broadcast_to(got['logz'][:, None], got['logw_out'].shape)[res]), what
    assert np.array_equal(got['ancestor'][~res], np.broadcast_to(np.arange(S), got['ancestor'].shape)[~res]), what
    # the ancestors of the groups both resampled
    rows = res & same
    ga, ra = got['ancestor'][rows], ref['ancestor'][rows]
    pinned = ref['margin'][rows] > ref['delta'][rows][:, None]
    assert np.array_equal(ga[pinned], ra[pinned]), (what, 'ancestors outside the margin', int((ga[pinned] != ra[pinned]).sum()))
    off = ga != ra
    assert np.all(np.abs(ga[off] - ra[off]) == 1), (what, 'inside the margin an ancestor moves by one')
    assert np.all(np.take_along_axis(ref['e'][rows], ga, axis=1) > 0), (what, 'an ancestor with e_n == 0')
    assert ga.size == 0 or (ga.min() >= 0 and ga.max() <= S - 1), what
    return int(off.sum())
