"""Float64 numpy statement of the weighted statistics, CRPS and quantiles of sample paths (include/snsde.h:
snsde_sample_stats_weighted, snsde_sample_crps_weighted, snsde_sample_quantiles_weighted and their adjoints), with first-order
round-off bounds derived from the summation order documented there.  Plain helpers, importable without a GPU.

Everything works on pooled sets: x (G, N, W) float32, logw (G, N) float32, y (G, W) float32.

Bounds, first order in the unit round-off u = 2^-24, times 1.01 for the higher orders.  With z_n = mx - a_n >= 0:
  e_n   = expf(fl(a_n - mx)): the rounded difference moves the exponent by z_n u, expf is within 3 ulp = 6 u:  rel. (z_n + 6) u
  P     a tree nine additions deep over non-negative terms:  rel. dP = sum e_n (z_n + 6) u / P + 9 u
  w_n   = fl(e_n / P):  |w^_n - w_n| <= EW_n := w_n ((z_n + 6) u + dP + u)
  t_n   = fl(w fl(1 - w)):  ET_n := EW_n (1 - w_n) + w_n (EW_n + u (1 - w_n)) + u t_n;   D' by the same tree:  ED := sum ET_n + 9 u D'
A chain of K fused multiply-adds of non-negative-sized terms s_k adds at most u K sum |s_k| to the errors of its terms.
  statistics  mean: sum_n EW_n |x_n| + u S sum |w x|.   d = fl(x - mean^): E_mean + u |d|;  fl(d d): sq := 2 |d| E_mean + E_mean^2
              + 3 u d^2 (the second-order E_mean^2 is kept: it is all there is where the samples are equal);
              ss: sum (EW_n d^2 + w_n sq_n) + u S ss;   var = fl(ss / D'): ESS / D' + var (ED / D' + u).
  CRPS        L_n, U_n are chains of at most N additions of w^_j: EC_n := sum_j EW_j + u (N + 1) (L_n + U_n).  A quarter chain and
              the three additions across quarters make K = ceil(N / 4) + 3.  A: sum (EW_n + u w_n) |d_n| + u K A;
              B: sum (|w C d| (rel_n + 3 u) + w_n EC_n |d_n|) + u K sum |w C d|;  crps = fl(A - fl(B / D)).
  quantiles   A_n a chain: EA_n := sum_(j before n) EW_j + u N A_n;  p_n = fl(A / fl(1 - w)):
              EP_n := (EA_n + p_n (EW_n + u (1 - w_n))) / (1 - w_n) + u p_n; the end nodes are exact by definition.
              A bracket is pinned where |q - p_k| > EP_k at every interior node k; q = 0 and q = 1 are pinned by the end nodes
              (exact values).  The value is a piecewise-linear function of q whose nodes move by at most EP: over the segment of
              the level and its two neighbours, each segment s = (a, b) contributes |x_b - x_a| min(1, 2 (EP_a + EP_b) / (p_b - p_a)),
              plus 4 u of the magnitudes for the arithmetic.  (1 - w_n loses everything where one weight dominates: EP says so.)"""
import numpy as np

U32 = 2.0 ** -24
INF = float('inf')
SLACK = 1.01
TINY = 1e-300

# (G, N, W) of the kernel tests (the issue's table): non-fair only; the smallest fair score; odd sizes with an uneven quarter split;
# three column tiles, the last with two live lanes; the LDS cap; the grid stride
SHAPES = [(1, 1, 1), (1, 2, 1), (3, 5, 33), (2, 64, 130), (1, 256, 4), (9000, 3, 2)]
POOLED = (2, 3, 2, 4, 6)              # (outer, M, G, S, W): members pooled and a leading axis
SCALES = (1.0, 4.0)                   # log-weights ~ N(0, 1) and N(0, 16)
LEVELS = (0.0, 0.1, 0.5, 0.9, 1.0)
SHARE_CAP = 0.02                      # of the (level, group, column) entries of a shape whose bracket cannot be pinned


def make_case(shape, scale, seed=0, ties=True):
    """Seeded float32 inputs of a (G, N, W) shape: x, logw ~ N(0, scale^2), y, and upstream gradients.  With ties=True sample 1
    duplicates sample 0 and the observation equals sample 2 (where the set has them)."""
    G, N, W = shape
    rng = np.random.default_rng(1000003 * seed + 7919 * G + 31 * N + W + int(100 * scale))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, logw, y = f(G, N, W), (scale * f(G, N)).astype(np.float32), f(G, W)
    if ties and N > 1:
        x[:, 1] = x[:, 0]
    if ties and N > 2:
        y = x[:, 2].copy()
    return dict(x=x, logw=logw, y=y, g=f(G, W), g2=f(G, W), gq=f(len(LEVELS), G, W))


def weights(logw, unit=U32):
    """(G, N) log-weights -> dict: w, live, bad (G), Dp (G), and the bounds EW (G, N), ED (G), rel (G, N)."""
    a = np.asarray(logw, np.float64)
    with np.errstate(all='ignore'):
        mx = np.max(np.where(np.isnan(a), -INF, a), axis=1, keepdims=True)
        e = np.exp(a - mx)
        P = e.sum(1, keepdims=True)
        bad = np.isnan(P[:, 0])
        live = ~((e == 0) & ~bad[:, None])
        w = e / P
        z = np.where(live & ~bad[:, None], mx - a, 0.0)
        rel_e = (z + 6.0) * unit
        dP = (np.where(live, e * rel_e, 0.0)).sum(1, keepdims=True) / P + 9.0 * unit
        rel = rel_e + dP + unit
        EW = np.where(live, w * rel, 0.0)
        t = w * (1.0 - w)
        ET = EW * (1.0 - w) + w * (EW + unit * (1.0 - w)) + unit * t
        Dp = t.sum(1)
        ED = ET.sum(1) + 9.0 * unit * Dp
    return dict(w=w, live=live, bad=bad, Dp=Dp, EW=EW, ED=ED, rel=rel)


def stats(x, logw, gm=None, gv=None, unit=U32, chain=None):
    """Weighted mean and variance (G, W) with bounds E_mean, E_var; with gm (and gv) also grad (G, N, W) and its bound E_grad."""
    wt = weights(logw, unit)
    w, live = wt['w'][:, :, None], wt['live'][:, :, None]
    EW = wt['EW'][:, :, None]
    S = chain or x.shape[1]      # (chain: the N of the kernel's call where x is that set with its dead samples removed)
    with np.errstate(all='ignore'):
        xs = np.where(live, np.asarray(x, np.float64), 0.0)
        mean = (w * xs).sum(1)
        E_mean = SLACK * ((EW * np.abs(xs)).sum(1) + unit * S * (w * np.abs(xs)).sum(1)) + TINY
        d = np.where(live, xs - mean[:, None], 0.0)
        ss = (w * d * d).sum(1)
        Dp, ED = wt['Dp'][:, None], wt['ED'][:, None]
        var = ss / Dp
        sq = 2.0 * np.abs(d) * E_mean[:, None] + E_mean[:, None] ** 2 + 3.0 * unit * d * d      # (E_mean^2: all that is left where d = 0)
        ESS = (EW * d * d + w * sq).sum(1) + unit * S * ss
        E_var = SLACK * (ESS / Dp + np.abs(var) * (ED / Dp + unit)) + TINY
        out = dict(mean=mean, var=var, E_mean=E_mean, E_var=E_var, wt=wt)
        if gm is not None:
            gm64 = np.asarray(gm, np.float64)[:, None]
            if gv is None:
                inner, E_in = np.broadcast_to(gm64, xs.shape), 0.0
            else:
                c = 2.0 * np.asarray(gv, np.float64)[:, None] / Dp[:, None]
                dc = ED[:, None] / Dp[:, None] + unit
                inner = c * d + gm64
                E_in = np.abs(c * d) * (dc + 2.0 * unit) + np.abs(c) * E_mean[:, None] + unit * (np.abs(c * d) + np.abs(gm64))
            out['grad'] = np.where(live, w * inner, 0.0)
            out['E_grad'] = SLACK * np.where(live, EW * np.abs(inner) + w * E_in + unit * w * np.abs(inner), 0.0) + TINY
    return out


def crps(x, logw, y, fair, g=None, unit=U32, chain=None):
    """Weighted CRPS, rank and ties (G, W) with bounds; with g also grad_x (G, N, W), grad_y (G, W) and their bounds."""
    wt = weights(logw, unit)
    w2, live2, EW2 = wt['w'], wt['live'], wt['EW']
    w, live, EW, rel = w2[:, :, None], live2[:, :, None], EW2[:, :, None], wt['rel'][:, :, None]
    G, N, W = x.shape
    NC = chain or N
    K = -(-NC // 4) + 3
    with np.errstate(all='ignore'):
        xs = np.where(live, np.asarray(x, np.float64), 0.0)
        wl = np.where(live2, w2, 0.0)
        lt = xs[:, None, :, :] < xs[:, :, None, :]                 # [g, n, j, w]: x_j < x_n
        gt = xs[:, None, :, :] > xs[:, :, None, :]
        L = (lt * wl[:, None, :, None]).sum(2)
        U = (gt * wl[:, None, :, None]).sum(2)
        C = L - U
        EC = EW2.sum(1)[:, None, None] + unit * (NC + 1) * (L + U)
        d = xs - np.asarray(y, np.float64)[:, None]
        if fair:
            D, ED = wt['Dp'][:, None], wt['ED'][:, None]
        else:
            D, ED = np.ones((G, 1)), np.zeros((G, 1))
        A = (wl[:, :, None] * np.abs(d)).sum(1)
        wcd = np.where(live, w * C * d, 0.0)
        B = wcd.sum(1)
        val = A - B / D
        EA = ((EW + unit * wl[:, :, None]) * np.abs(d)).sum(1) + unit * K * A
        EB = (np.abs(wcd) * (rel + 3.0 * unit) + wl[:, :, None] * EC * np.abs(d)).sum(1) + unit * K * np.abs(wcd).sum(1)
        E_val = SLACK * (EA + EB / D + np.abs(B / D) * (ED / D + unit) + unit * np.abs(val)) + TINY
        below, equal = (wl[:, :, None] * (d < 0)).sum(1), (wl[:, :, None] * (d == 0)).sum(1)
        E_rank = SLACK * ((EW * (d < 0)).sum(1) + unit * K * below) + TINY
        E_ties = SLACK * ((EW * (d == 0)).sum(1) + unit * K * equal) + TINY
        nanrow = wt['bad'][:, None]
        val, below, equal = (np.where(nanrow, np.nan, v) for v in (val, below, equal))
        out = dict(crps=val, rank=below, ties=equal, E_crps=E_val, E_rank=E_rank, E_ties=E_ties, wt=wt)
        if g is not None:
            g64 = np.asarray(g, np.float64)
            sg = np.sign(d)
            q = C / D[:, None]
            Eq = EC / D[:, None] + np.abs(q) * (ED[:, None] / D[:, None] + unit)
            inner = sg - q
            out['grad_x'] = np.where(live, g64[:, None] * w * inner, 0.0)
            out['E_grad_x'] = SLACK * np.abs(g64[:, None]) * np.where(live, EW * np.abs(inner) + w * Eq + 3.0 * unit * w * np.abs(inner), 0.0) + TINY
            s = (wl[:, :, None] * sg).sum(1)
            out['grad_y'] = -g64 * s
            out['E_grad_y'] = SLACK * np.abs(g64) * ((EW * np.abs(sg)).sum(1) + unit * K * (wl[:, :, None] * np.abs(sg)).sum(1) + unit * np.abs(s)) + TINY
            if wt['bad'].any():
                for k in ('grad_x', 'grad_y'):
                    out[k] = np.where(wt['bad'].reshape((G,) + (1,) * (out[k].ndim - 1)), np.nan, out[k])
    return out


def quantiles(x, logw, levels=LEVELS, gq=None, unit=U32, chain=None):
    """Weighted quantiles (Q, G, W) with the bound E, pinned (Q, G, W), lo / hi sample indices and frac; with gq (Q, G, W) also
    grad (G, N, W), its bound, and col_pinned (G, W): every level of the column pinned."""
    wt = weights(logw, unit)
    G, N, W = x.shape
    qs = np.asarray([np.float32(v) for v in levels], np.float64)
    Q = len(qs)
    with np.errstate(all='ignore'):
        live = np.broadcast_to(wt['live'][:, None, :], (G, W, N))
        xt = np.where(live, np.asarray(x, np.float64).transpose(0, 2, 1), 0.0)          # (G, W, N)
        has_nan = (np.isnan(xt) & live).any(-1)
        key = np.where(np.isnan(xt), 0.0, xt)
        first = np.argsort(key, axis=-1, kind='stable')
        order = np.take_along_axis(first, np.argsort(np.take_along_axis(~live, first, -1), axis=-1, kind='stable'), -1)   # the live first
        ws = np.take_along_axis(np.broadcast_to(wt['w'][:, None, :], (G, W, N)), order, -1)
        ews = np.take_along_axis(np.broadcast_to(wt['EW'][:, None, :], (G, W, N)), order, -1)
        xs = np.take_along_axis(xt, order, -1)
        F = wt['live'].sum(1)[:, None, None]
        r = np.broadcast_to(np.arange(N), (G, W, N))
        before = lambda v: np.concatenate((np.zeros_like(v[..., :1]), np.cumsum(v, -1)[..., :-1]), -1)      # (no cancellation)
        A = before(ws)
        EA = before(ews) + unit * (chain or N) * A
        p = A / (1.0 - ws)
        EP = (EA + p * (ews + unit * (1.0 - ws))) / (1.0 - ws) + unit * p
        ends = (r == 0) | (r == F - 1)
        p = np.where(r == F - 1, 1.0, p)
        p = np.where(r == 0, 0.0, p)
        EP = np.where(ends, 0.0, EP)
        ranked = r < F
        p = np.where(ranked, p, INF)
        EP = np.where(ranked, EP, 0.0)
        val, E, pinned = np.empty((Q, G, W)), np.empty((Q, G, W)), np.empty((Q, G, W), bool)
        los, his, fracs = np.empty((Q, G, W), np.int64), np.empty((Q, G, W), np.int64), np.empty((Q, G, W))
        EFs = np.empty((Q, G, W))
        bad = wt['bad'][:, None]
        take = lambda arr, i: np.take_along_axis(arr, i[..., None], -1)[..., 0]
        for i, q in enumerate(qs):
            lo = np.where(p <= q, r, 0).max(-1)
            last = lo == F[..., 0] - 1
            hi = np.minimum(lo + 1, N - 1)
            plo, phi, xlo, xhi = take(p, lo), take(p, hi), take(xs, lo), take(xs, hi)
            den = phi - plo
            frac = np.where(last, 0.0, np.clip((q - plo) / den, 0.0, 1.0))
            v = np.where(last | (frac == 0), xlo, xlo + frac * (np.where(last, xlo, xhi) - xlo))
            pinned[i] = ((EP == 0) | (np.abs(q - p) > SLACK * EP) | ~ranked).all(-1)
            bound = 4.0 * unit * (np.abs(xlo) + np.where(last, 0.0, np.abs(xhi)))
            for s in (-1, 0, 1):                                  # the segment (lo + s, lo + s + 1), where it exists
                a_, b_ = lo + s, lo + s + 1
                ok = (a_ >= 0) & (b_ <= F[..., 0] - 1)
                a_, b_ = np.clip(a_, 0, N - 1), np.clip(b_, 0, N - 1)
                seg = take(p, b_) - take(p, a_)
                move = 2.0 * (take(EP, a_) + take(EP, b_))
                share = np.where(seg > 0, np.minimum(1.0, move / np.where(seg > 0, seg, 1.0)), 1.0)
                bound = bound + np.where(ok, np.abs(take(xs, b_) - take(xs, a_)) * share, 0.0)
            if q == 0.0 or q == 1.0:      # the end nodes are exact by definition: rank 0 (frac = 0) and rank F - 1, whatever the rounding
                pinned[i], bound = True, np.zeros_like(bound)
            EPlo, EPhi = take(EP, lo), take(EP, hi)
            EFs[i] = np.where(last, 0.0, (EPlo + unit * np.abs(q - plo)) / den + frac * (EPlo + EPhi + unit * den) / den + unit * frac)
            val[i] = np.where(has_nan | bad, np.nan, v)
            E[i] = SLACK * bound + TINY
            los[i], his[i], fracs[i] = take(order, lo), np.where(last | (frac == 0), -1, take(order, hi)), frac
        out = dict(out=val, E=E, pinned=pinned | has_nan[None] | bad[None], lo=los, hi=his, frac=fracs, has_nan=has_nan, wt=wt)
        if gq is not None:
            g64 = np.asarray(gq, np.float64)
            grad, Eg = np.zeros((G, W, N)), np.zeros((G, W, N))
            for i in range(Q):
                glo, ghi = g64[i] * (1.0 - fracs[i]), g64[i] * fracs[i]
                eg = np.abs(g64[i]) * (EFs[i] + 3.0 * unit)
                np.add.at(grad, (*np.indices((G, W)), los[i]), glo)
                np.add.at(Eg, (*np.indices((G, W)), los[i]), eg)
                m = his[i] >= 0
                gi, wi = np.nonzero(m)
                np.add.at(grad, (gi, wi, his[i][m]), ghi[m])
                np.add.at(Eg, (gi, wi, his[i][m]), eg[m])
            grad = np.where(has_nan[..., None], 0.0, grad)
            grad = np.where(bad[..., None], np.nan, grad)
            out['grad'] = grad.transpose(0, 2, 1)
            out['E_grad'] = (SLACK * (Eg + unit * Q * np.abs(grad)) + TINY).transpose(0, 2, 1)
            out['col_pinned'] = out['pinned'].all(0)
    return out


def pool(ys, M, S):
    """(outer, M, G S, W) -> (outer G, M S, W), n = m S + s (members = 1: ys (outer, G S, W))."""
    o, G, W = ys.shape[0], ys.shape[-2] // S, ys.shape[-1]
    return ys.reshape(o, M, G, S, W).transpose(0, 2, 1, 3, 4).reshape(o * G, M * S, W)


def unpool(xg, o, M, S):
    """The inverse of `pool`: (outer G, M S, W) -> (outer, M, G S, W)."""
    G, W = xg.shape[0] // o, xg.shape[-1]
    return xg.reshape(o, G, M, S, W).transpose(0, 2, 1, 3, 4).reshape(o, M, G * S, W)


def ratio(got, ref, bound):
    """max |got - ref| / bound over the finite reference entries; NaN-ness and infinities must agree exactly."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), 'NaN pattern differs'
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), 'infinite entries differ'
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.broadcast_to(bound, ref.shape)[fin]).max())
