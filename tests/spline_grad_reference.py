"""float64 restatement of the adjoints of the two spline constructions, and the cases the spline-gradient tests share.

Both constructions are linear in the observed values of X: the compaction of observed knots, the tridiagonal matrix, the end
imputation, the fill weights and the re-expansion offsets depend on `times` and on which entries are NaN only.  So
grad_X = J^T grad_coeffs needs the mask of X and nothing else of the forward.  `natural_backward` / `hermite_backward` state
the two transposes series by series in numpy float64; tests/test_spline_grad_cpu.py pins them against torch.autograd through the
package's tensor-op constructions, tests/test_gpu_spline_grad.py compares the HIP kernels with the same autograd gradient.

Layout: times (L,), X (B, L, C) with NaN = missing, grad_coeffs (B, L-1, 4C) = cotangent of cat[a, b, two_c, three_d],
result (B, L, C) with exact zeros at missing entries."""
import numpy as np
import torch

import stable_neural_sdes_amd as S

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0, 6.5, 8.0])
KNOTS = (9, 2, 3)
SHAPES = ((3, 5), (7, 21))       # (7, 21): 147 series = one full workgroup of 128 and a ragged second one
KINDS = ('natural', 'hermite')
NAN_FRAC = 0.3


# ---- the natural spline --------------------------------------------------------------------------------------------------

def _natural_series(t, obs, g):
    """One series.  t (L,), obs (L,) bool, g (L-1, 4) cotangents of (a, b, two_c, three_d)  ->  (L,)."""
    L = t.shape[0]
    out = np.zeros(L)
    if not obs.any():
        return out
    first, last = int(np.flatnonzero(obs)[0]), int(np.flatnonzero(obs)[-1])
    oidx = [j for j in range(L) if obs[j] or j == 0 or j == L - 1]      # the ends are always knots (imputed when missing)
    m = len(oidx)
    tc = t[oidx]
    # transpose of the re-expansion: original interval j lies in compressed interval p, off = tc_p - t_j
    gA, gBc, gC2, gD3 = np.zeros(m - 1), np.zeros(m - 1), np.zeros(m - 1), np.zeros(m - 1)
    for p in range(m - 1):
        for j in range(oidx[p], oidx[p + 1]):
            off = tc[p] - t[j]
            ga, gb, gc, gd = g[j]
            gA[p] += ga
            gBc[p] += gb - ga * off
            gC2[p] += ga * off ** 2 / 2 - gb * off + gc
            gD3[p] += -ga * off ** 3 / 3 + gb * off ** 2 - 2 * gc * off + gd
    gdx = np.zeros(m - 1)
    if m == 2:           # A = x0, Bc = (x1 - x0) / (tc_1 - tc_0), C2 = D3 = 0
        gdx[0] = gBc[0] / (tc[1] - tc[0])
    else:
        rec = 1.0 / (tc[1:] - tc[:-1])
        # C2 = (6 dx rec - 4 k_p - 2 k_{p+1}) rec,  D3 = (-6 dx rec + 3 (k_p + k_{p+1})) rec^2,  Bc = k_p
        gk = np.zeros(m)
        gk[:-1] += gBc - 4 * rec * gC2 + 3 * rec ** 2 * gD3
        gk[1:] += -2 * rec * gC2 + 3 * rec ** 2 * gD3
        gdx += 6 * rec ** 2 * gC2 - 6 * rec ** 3 * gD3
        # k = T^-1 rhs with T symmetric: g rhs = T^-1 gk
        T = np.zeros((m, m))
        for i in range(m):
            T[i, i] = 2 * ((rec[i - 1] if i > 0 else 0.0) + (rec[i] if i < m - 1 else 0.0))
            if i < m - 1:
                T[i, i + 1] = T[i + 1, i] = rec[i]
        u = np.linalg.solve(T, gk)
        # rhs_i = sc_{i-1} + sc_i,  sc_i = 3 dx_i rec_i^2
        gdx += 3 * rec ** 2 * (u[:-1] + u[1:])
    gxc = np.zeros(m)
    gxc[:-1] += gA - gdx
    gxc[1:] += gdx
    for i, j in enumerate(oidx):
        if obs[j]:
            out[j] += gxc[i]
        else:                # an imputed end: xc = the first (j = 0) or the last (j = L-1) observation
            out[first if j == 0 else last] += gxc[i]
    return out


# ---- the Hermite spline with backward differences ---------------------------------------------------------------------------

def _hermite_series(t, obs, g):
    L = t.shape[0]
    h = t[1:] - t[:-1]
    # c_j = 4 (m_j - b_j) / h_j, d_j = -3 (m_j - b_j) / h_j^2, b_j = m_{j-1} (b_0 = m_0), a_j = xf_j, m_j = (xf_{j+1} - xf_j) / h_j
    s = 4 * g[:, 2] / h - 3 * g[:, 3] / h ** 2        # cotangent of (m_j - b_j)
    gb = g[:, 1] - s                                  # cotangent of b_j
    gm = s.copy()
    gm[0] += gb[0]
    gm[:-1] += gb[1:]
    gxf = np.zeros(L)
    gxf[:-1] += g[:, 0] - gm / h
    gxf[1:] += gm / h
    out = np.zeros(L)
    if not obs.any():
        return out
    where = np.flatnonzero(obs)
    for j in range(L):
        if obs[j]:
            out[j] += gxf[j]
            continue
        prev, nxt = where[where < j], where[where > j]
        if prev.size == 0:
            out[nxt[0]] += gxf[j]                     # leading gap: the next observation
        elif nxt.size == 0:
            out[prev[-1]] += gxf[j]                   # trailing gap: the previous one
        else:
            pj, nj = prev[-1], nxt[0]
            w = (t[j] - t[pj]) / (t[nj] - t[pj])
            out[pj] += (1 - w) * gxf[j]
            out[nj] += w * gxf[j]
    return out


def _backward(series, times, X, grad_coeffs):
    t = np.asarray(times, np.float64)
    X = np.asarray(X)
    g = np.asarray(grad_coeffs, np.float64)
    B, L, Cn = X.shape
    out = np.zeros((B, L, Cn))
    for b in range(B):
        for c in range(Cn):
            out[b, :, c] = series(t, ~np.isnan(X[b, :, c]), g[b][:, c::Cn])
    return out


def natural_backward(times, X, grad_coeffs):
    return _backward(_natural_series, times, X, grad_coeffs)


def hermite_backward(times, X, grad_coeffs):
    return _backward(_hermite_series, times, X, grad_coeffs)


RESTATEMENT = {'natural': natural_backward, 'hermite': hermite_backward}


# ---- the cases ---------------------------------------------------------------------------------------------------------------

def _patterns(L):
    """Observed-entry masks planted in fixed series (the rest gets NAN_FRAC random NaN); at L = 2 / 3 what fits."""
    full = np.ones(L, bool)

    def only(*idx):
        mk = np.zeros(L, bool)
        mk[[i for i in idx if 0 <= i < L]] = True
        return mk

    def without(*idx):
        mk = full.copy()
        mk[[i for i in idx if 0 <= i < L]] = False
        return mk

    pats = [('no NaN', full),
            ('interior gaps', without(1, 2, 5) if L > 3 else without(1)),
            ('first missing', without(0)),
            ('last missing', without(L - 1)),
            ('both ends missing', without(0, L - 1) if L > 2 else without(0)),
            ('one observation, interior', only(L // 2)),
            ('one observation, first', only(0)),
            ('one observation, last', only(L - 1)),
            ('two observations at the ends (m == 2)', only(0, L - 1)),
            ('two observations inside', only(2, 6) if L > 6 else only(0, 1)),
            ('first two missing, last two missing', without(0, 1, L - 2, L - 1) if L > 4 else without(0)),
            ('no observation', np.zeros(L, bool))]
    return pats


_CASES = {}


def case(L, B, Cn):
    """times, X (float64, NaN planted), cotangent g, the names of the planted series: built once, shared, never modified."""
    key = (L, B, Cn)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 + 100 * L + 10 * B + Cn)
    X = rng.standard_normal((B, L, Cn)).cumsum(axis=1)
    X[rng.random((B, L, Cn)) < NAN_FRAC] = np.nan
    vals = rng.standard_normal((B, L, Cn)).cumsum(axis=1)
    planted = {}
    pats = _patterns(L)
    starts = [0] + ([128] if B * Cn >= 128 + len(pats) else [])      # also in the ragged second workgroup
    for s0 in starts:
        for k, (name, mk) in enumerate(pats):
            b, c = divmod(s0 + k, Cn)
            X[b, :, c] = np.where(mk, vals[b, :, c], np.nan)
            planted[(b, c)] = name
    g = rng.standard_normal((B, L - 1, 4 * Cn))
    c = dict(L=L, B=B, C=Cn, times=TIMES[:L].copy(), X=X, g=g, planted=planted)
    _CASES[key] = c
    return c


CASE_KEYS = [(L, B, Cn) for L in KNOTS for (B, Cn) in SHAPES]


def tensor_op_coeffs(kind, times, X):
    """The package's tensor-op construction (CPU tensors take it; so does any float64 tensor), packed (B, L-1, 4C)."""
    if kind == 'natural':
        return torch.cat(S.controldiffeq.natural_cubic_spline_coeffs(times, X), dim=-1)
    return S.torchcde.hermite_cubic_coefficients_with_backward_differences(X, times)


_AUTOGRAD = {}


def autograd_gradient(kind, key, dtype=torch.float64):
    """grad_X of <g, coeffs> by torch.autograd through the tensor-op construction on the CPU (float64: the reference of every
    test; float32: the yardstick of the GPU test's bound).  Cached."""
    k = (kind, key, dtype)
    if k not in _AUTOGRAD:
        c = case(*key)
        X = torch.from_numpy(c['X']).to(dtype).requires_grad_(True)
        out = tensor_op_coeffs(kind, torch.from_numpy(c['times']).to(dtype), X)
        (gx,) = torch.autograd.grad((out * torch.from_numpy(c['g']).to(dtype)).sum(), X)
        _AUTOGRAD[k] = gx.detach()
    return _AUTOGRAD[k]
