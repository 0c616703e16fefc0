"""Float64 numpy statement of the energy score of weighted, partially observed sample sets (include/snsde.h:
snsde_sample_energy_weighted and its adjoint), with first-order round-off bounds derived from the summation order documented
there.  Plain helpers, importable without a GPU.

Everything works on pooled sets: x (G, N, V) float32, y (G, V) float32, logw (G, N) float32 or None, obs (G, V) bool or None (a
coordinate is observed where True), g (G,) float32 upstream gradients.

Definitions.  With O the observed coordinates of a score, (w, live, D') the normalised weights of tests/sample_weighted_reference
(`weights`: mx, e_n, P, w_n = e_n / P, D' = sum w_n (1 - w_n); dead where e_n == 0 and P is a number; P = NaN: every w_n NaN),
    r_n = ||(x_n - y)|_O||,  r_nj = ||(x_n - x_j)|_O||,  u(d) = d|_O / ||d|_O||, u(0) = 0
    energy      = sum_n w_n r_n - sum_{n<j} w_n w_j r_nj / D            D = D' (fair) or 1; live n, j only
    grad_x[n]   = g (w_n u(x_n - y) - sum_{j != n} w_n w_j u(x_n - x_j) / D)
    grad_y      = -g sum_n w_n u(x_n - y)
without weights w_n = 1 / N and D = (N - 1) / N (fair) or 1.  Gradients at unobserved coordinates and in the rows of dead samples
are exact zeros.  A group with P = NaN is NaN (zeros at its unobserved coordinates).  One live sample under fair: D' = 0 and the
sums over no pair are 0 / 0 = NaN, in the value and in that sample's gradient.

Bounds, first order in u = 2^-24, times 1.01 for the higher orders.
  distance  a chain of fmaf over the Vo observed columns (an unobserved column adds fmaf(0, 0, .): exact) of once-rounded
            differences: the square within (Vo + 2) u, sqrtf halves it and rounds once: r within dr = (Vo / 2 + 2) u, relative.
  weights   |w^_n - w_n| <= w_n rho_n, rho_n = (z_n + 6) u + dP + u with expf at 3 ulp (`weights`: rel, EW); D' within ED.
  value     the term of a pair is fl(fl(w_i w_j) r): relative rho_i + rho_j + dr + 2 u (the observation has w = 1, rho = 0).  The
            documented order adds the terms of each of the two sums through 4 tree levels of a tile, at most 9 tiles of a lane, 6
            butterfly levels and 3 waves, masked and dead pairs as exact zeros: never deeper than min(#terms - 1, 22) <= 2 N
            additions.  fl(B / D^) adds ED / D' + u, the subtraction u: with the unweighted kernel's divisions by N and N D in place
            of the products this is the (V / 2 + 2 N + 8) u (A + B') of the unweighted score, so
                E = (Vo / 2 + 2 N + 8) u (A + B / D) + sum_n w_n rho_n r_n + sum_{n<j} w_n w_j (rho_n + rho_j) r_nj / D + (B / D) ED / D
  gradient  a plane entry is fl(fl(1 / r) c): 1 / r carries dr + u; c = fl(w_i w_j) with the observation, fl(fl(w_i w_j) fl(-1 / D^))
            among samples: rho_i + rho_j + ED / D' + 3 u; the product u; each term one rounded difference u; the N terms of a row
            one fmaf each: N u; the product with g: u.  That is (Vo / 2 + N + 10) u with weights - (Vo / 2 + N + 8) u without, the
            unweighted adjoint's bound, whose entries are 1 / N and 1 / (N D) - times the sum of the magnitudes, |u_v| <= 1:
                E_x[n] = |g| (c_u s_n + w_n rho_n + sum_j w_n w_j (rho_n + rho_j + ED / D) / D),  s_n = w_n + sum_{j != n} w_n w_j / D
                E_y    = |g| (c_u + sum_n w_n rho_n),   c_u = (Vo / 2 + N + 10 or 8) u"""
import numpy as np

from tests import sample_weighted_reference as R

U32 = R.U32
SLACK, TINY = R.SLACK, R.TINY

# (scores, N, V): the small shapes of the unweighted GPU test - either side of each bucket edge (39 | 40, 87 | 88, 151 | 152), a
# row block (N + 1 = 65 | 66), a chunk boundary with one live tail column, the cap
SHAPES = [(1, 2, 1), (3, 5, 3), (2, 39, 5), (2, 40, 5), (2, 64, 65), (2, 65, 130), (1, 87, 4), (1, 88, 4), (1, 151, 4), (1, 152, 4),
          (1, 256, 4), (2, 3, 17)]
SCALES = (1.0, 4.0)                   # log-weights ~ N(0, 1) and N(0, 16)
MASK_SHARE = 0.4                      # of the coordinates of a masked case that are gaps


def make_case(shape, scale=None, masked=False, seed=0, ties=True):
    """Seeded float32 inputs of a (G, N, V) shape: x, y, g, logw ~ N(0, scale^2) (None without scale) and obs (None unless masked:
    about 40 % gaps, whose x and y entries are then poisoned with NaN / Inf).  With ties=True sample 1 duplicates sample 0 and the
    observation equals sample 2 (where the set has them)."""
    G, N, V = shape
    rng = np.random.default_rng(1000003 * seed + 7919 * G + 31 * N + V + int(100 * (scale or 0)) + (5 if masked else 0))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, y, g = (2.0 * f(G, N, V) + 0.5).astype(np.float32), f(G, V), f(G)
    if ties and N > 1:
        x[:, 1] = x[:, 0]
    if ties and N > 2:
        y = x[:, 2].copy()
    logw = None if scale is None else (scale * f(G, N)).astype(np.float32)
    obs = None
    if masked:
        obs = rng.random((G, V)) >= MASK_SHARE
        obs[np.arange(G), rng.integers(V, size=G)] = True      # (every score keeps a column; nothing observed is a case of its own)
        x = np.where(obs[:, None, :], x, np.where(rng.random((G, N, V)) < 0.5, np.nan, np.inf)).astype(np.float32)
        y = np.where(obs, y, np.nan).astype(np.float32)
    return dict(x=x, y=y, g=g, logw=logw, obs=obs)


def energy(x, y, logw=None, obs=None, fair=True, g=None, unit=U32):
    """-> dict: energy (G,) and its bound E; with g also grad_x (G, N, V), grad_y (G, V) and their bounds E_x, E_y."""
    G, N, V = x.shape
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if obs is None:
        obs = np.ones((G, V), bool)
    with np.errstate(all='ignore'):
        if logw is None:
            w, live, bad = np.full((G, N), 1.0 / N), np.ones((G, N), bool), np.zeros(G, bool)
            rho, D, ED = np.zeros((G, N)), np.full(G, (N - 1.0) / N if fair else 1.0), np.zeros(G)
        else:
            wt = R.weights(logw, unit)
            w, live, bad = wt['w'], wt['live'] & ~wt['bad'][:, None], wt['bad']
            rho = np.where(live, wt['rel'], 0.0)
            D, ED = (wt['Dp'], wt['ED']) if fair else (np.ones(G), np.zeros(G))
        keep = obs[:, None, :] & live[:, :, None]
        xs, ys = np.where(keep, x64, 0.0), np.where(obs, y64, 0.0)
        wl = np.where(live, w, 0.0)
        Vo = obs.sum(1).astype(np.float64)
        d = np.where(keep, xs - ys[:, None], 0.0)                             # (G, N, V)
        rn = np.sqrt((d * d).sum(-1))                                         # (G, N)
        diff = np.where(keep[:, :, None] & keep[:, None, :], xs[:, :, None] - xs[:, None, :], 0.0)      # (G, N, N, V)
        rnj = np.sqrt((diff * diff).sum(-1))                                  # (G, N, N)
        ww = wl[:, :, None] * wl[:, None, :]
        off = ~np.eye(N, dtype=bool)[None]
        A = (wl * rn).sum(1)
        B = (ww * rnj * off).sum((1, 2)) / 2.0                                # (the full plane counts every pair twice)
        pairs = (live[:, :, None] & live[:, None, :] & off).sum((1, 2)) > 0
        BD = np.where(pairs, B, 0.0) / np.where(pairs, D, 1.0) + np.where(pairs | (D != 0), 0.0, np.nan)      # (no pair over D' = 0: 0 / 0)
        val = A - BD
        rr = rho[:, :, None] + rho[:, None, :]
        relD = np.where(D > 0, ED / np.where(D > 0, D, 1.0), 0.0)
        E = SLACK * ((Vo / 2 + 2 * N + 8) * unit * (A + np.abs(BD)) + (wl * rho * rn).sum(1)
                     + np.where(pairs, (ww * rr * rnj * off).sum((1, 2)) / 2.0 / np.where(D > 0, D, 1.0), 0.0) + np.abs(BD) * relD) + TINY
        val = np.where(bad, np.nan, val)
        out = dict(energy=val, E=E, A=A, B=BD, live=live, bad=bad, obs=obs)
        if g is not None:
            g64 = np.asarray(g, np.float64)
            un = np.where(rn[..., None] > 0, d / np.where(rn[..., None] > 0, rn[..., None], 1.0), 0.0)
            unj = np.where(rnj[..., None] > 0, diff / np.where(rnj[..., None] > 0, rnj[..., None], 1.0), 0.0)
            others = (live[:, :, None] & live[:, None, :] & off)              # [g, n, j]: a live j != n for a live n
            invD = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), np.where(logw is None, 0.0, np.inf))
            second = (ww[..., None] * unj * others[..., None]).sum(2) * invD[:, None, None]
            second = second + np.where((D == 0)[:, None, None] & live[:, :, None], np.nan, 0.0)      # (the formula's 0 / 0)
            gx = g64[:, None, None] * (wl[:, :, None] * un - second)
            gy = -g64[:, None] * (wl[:, :, None] * un).sum(1)
            cu = (Vo / 2 + N + (8 if logw is None else 10)) * unit
            Dn = np.where(D > 0, D, 1.0)[:, None]
            sn = wl + (ww * others).sum(2) / Dn
            Ex = np.abs(g64)[:, None] * (cu[:, None] * sn + wl * rho + (ww * others * (rr + relD[:, None, None])).sum(2) / Dn)
            Ey = np.abs(g64) * (cu * wl.sum(1) + (wl * rho).sum(1))
            gx = np.where(keep, gx, 0.0)
            gy = np.where(obs, gy, 0.0)
            gx = np.where(bad[:, None, None] & obs[:, None, :], np.nan, gx)
            gy = np.where(bad[:, None] & obs, np.nan, gy)
            out.update(grad_x=gx, grad_y=gy, E_x=np.broadcast_to(SLACK * Ex[:, :, None] + TINY, gx.shape),
                       E_y=np.broadcast_to(SLACK * Ey[:, None] + TINY, gy.shape))
    return out


def set_observed(c, group, column, observed):
    """Make one coordinate of a (fresh, masked) case observed - with finite values in it - or a gap, in place."""
    c['obs'][group, column] = observed
    if observed:
        c['x'][group, :, column] = 0.5 + 0.25 * np.arange(c['x'].shape[1], dtype=np.float32)
        c['y'][group, column] = -0.75


def replicate(x, counts):
    """The sample set with sample n repeated counts[n] times: x (G, N, V), counts (N,) integers -> (G, sum counts, V)."""
    return np.repeat(x, np.asarray(counts), axis=1)


def compact(x, y, obs_row):
    """The vectors of one mask row compacted to their observed columns: x (G, N, V), y (G, V), obs_row (V,) -> (G, N, Vo), (G, Vo)."""
    return np.ascontiguousarray(x[:, :, obs_row]), np.ascontiguousarray(y[:, obs_row])


ratio = R.ratio
