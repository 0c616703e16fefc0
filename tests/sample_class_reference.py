"""Float64 numpy statement of snsde_sample_class / sample_class and of its adjoint, with error bounds derived from the summation
order include/snsde.h documents.  Shared by tests/test_sample_class_cpu.py and tests/test_gpu_sample_class.py; independent of
engine.sample_class_tensor_ops (no torch).

plan(N, C) restates the kernel's buckets: L = min(64, least power of two >= C) lanes per row, R = 256 / L rows at a time, GP
groups per workgroup (1 for C > 64, else the largest power of two <= max(1, R / N)), RS = min(16, R / GP) row parts of the
column sums (1 for C > 64), CP column lanes (L, or 256 for C > 64), TN = min(64, 256 / GP) lanes over the paths, and whether the
pack's slab (GP N C floats) is staged in LDS (<= 24576).

The bounds, u the unit round-off (2^-24 for the kernel, 2^-53 for the float64 statement), expf / logf within 2 ulp (4 u):
  row: z - m is exact or rounds within u |z - m|; a term expf(z - m) is rescaled along the lane's chain, and once more against
  the row's maximum, by factors whose exponents telescope to m_final - m, so its relative error is u (2 |z - m| + 5 D1 + 8)
  with D1 = ceil(C / L) + log2 L the depth of chain plus butterfly (products, sums and expf each counted, with room to
  spare: the rescaling products are at most ceil(C / L) + 1).  Weighted by the terms' shares p_c:
  s within (2 W + 5 D1 + 8) u relatively, W = sum_c p_c |z_c - m|; ls = logf(s) within E_ls = u (2 W + 5 D1 + 8 + 4 |ls|);
  lp_c = (z_c - m) - ls within E_lp = E_ls + u |z_c - m| + u |lp_c|.  logp = lp_y.
  nll: a'_n = logp_n + logw_n rounds once, E_a = E_logp + u |a'_n|; logsumexp is 1-Lipschitz in max_n E_a; its own arithmetic
  (as derived for snsde_sample_loglik): u (2 |max a'| + 11 log N + Dn + 16), Dn = ceil(N / TN) + log2 TN; the product with w
  and the subtraction 2 u |nll|.
  xent: the sum of N values each within E_logp, chain and butterfly Dn, the division and the product:
  |w| / N (sum_n E_logp + (Dn + 2) u sum_n |logp_n|) + 2 u |xent|.
  probs: p_nc = expf(lp_nc) within p (1.01 E_lp + 4 u) + TINY (float32 has no p below 2^-126); the parts, their sum and the
  division D2 = ceil(N / RS) + RS + 2 (C > 64: N + 2): mean_n E_p + D2 u pbar_c.
  entropy: h(p) = -p log p has |h'| = |log p + 1|: sum_c 1.01 (|log pbar_c| + 1) E_probs_c + 5 u |h_c|, and the sum over the
  classes D3 = log2 min(CP, 64) + ceil(C / CP) + 4: D3 u sum_c |h_c|.
  expent: a term p lp within E_p (|lp| + 1) + p E_lp + 2 u p |lp|; the sum of depth D4 = ceil(N / RS) ceil(C / CP) + RS +
  log2 min(CP, 64) + 4: (D4 + 2) u mean_n sum_c p |lp|.
  backward: r_n = expf(a'_n - max) / sum relatively within R = expm1(2 max_n (E_a + u |a'_n - max|)) + (Dn + 16) u, absolutely
  TINY more; k_n = w (grad_nll r_n + grad_xent / N) - grad_logp_n within |w grad_nll| E_r + 4 u (|w| (|grad_nll| r_n +
  |grad_xent| / N) + |grad_logp_n|) + TINY; grad_logits = k_n (p_nc - [c == y]) within E_k |p - d| + |k| (E_p + u |p - d|) +
  u |grad| + TINY; grad_logw = -w grad_nll r_n within |w grad_nll| (E_r + 3 u r_n) + TINY.
The tensor-op statement (ops=True): the same formulas with torch's sums no deeper than their length: D1 = C, Dn = N, D2 = N + 2,
D3 = C + 4, D4 = N C + 4."""
import math

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -126


def plan(N, C):
    L = 1
    while L < 64 and L < C:
        L *= 2
    R = 256 // L
    GP = 1
    if C <= 64:
        while 2 * GP * N <= R:
            GP *= 2
    RS = min(16, R // GP) if C <= 64 else 1
    CP = L if C <= 64 else 256
    TN = min(64, 256 // GP)
    return dict(L=L, R=R, GP=GP, RS=RS, CP=CP, TN=TN, staged=GP * N * C <= 24576)


def _xlogx(p):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p == 0, 0.0, p * np.log(p))


def reference(z, y, logw=None, cw=None, binary=False, grads=None, u=U32, tiny=TINY32, ops=False):
    """z (G, N, C) float64 logits (binary: C = 1), y (G,) integers or None, logw (G, N) or None, cw (classes,) or None.
    grads: None or (grad_nll (G,), grad_xent (G,), grad_logp (G, N)).  Returns a dict of values and their bounds E_*."""
    z = np.asarray(z, np.float64)
    G, N, Cw = z.shape
    pl = plan(N, Cw)
    z2 = np.concatenate([np.zeros_like(z), z], -1) if binary else z
    Cl = z2.shape[-1]
    y = np.full(G, -1, np.int64) if y is None else np.asarray(y, np.int64)
    lw = np.zeros((G, N)) if logw is None else np.asarray(logw, np.float64)
    if ops:
        D1, Dn, D2, D3, D4 = Cl, N, N + 2, Cl + 4, N * Cl + 4
    else:
        l2 = lambda v: int(math.log2(v))
        D1 = 2 if binary else -(-Cw // pl['L']) + l2(pl['L'])
        Dn = -(-N // pl['TN']) + l2(pl['TN'])
        D2 = (-(-N // pl['RS']) + pl['RS'] + 2) if Cw <= 64 else N + 2
        D3 = l2(min(pl['CP'], 64)) + -(-Cw // pl['CP']) + 4
        D4 = -(-N // pl['RS']) * -(-Cw // pl['CP']) + pl['RS'] + l2(min(pl['CP'], 64)) + 4
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        m = z2.max(-1, keepdims=True)
        msh = np.where(np.isneginf(m), 0.0, m)
        dz = z2 - msh
        s = np.exp(dz).sum(-1)
        ls = np.log(s)
        lp = dz - ls[..., None]
        p = np.exp(lp)
        dead = np.isneginf(lp)                                   # classes of probability zero: exact
        W = np.where(dead, 0.0, p * np.abs(dz)).sum(-1)
        E_ls = u * (2 * W + 5 * D1 + 8 + 4 * np.abs(ls))
        E_lp = np.where(dead, 0.0, E_ls[..., None] + u * np.abs(dz) + u * np.abs(lp))
        E_p = np.where(dead, 0.0, p * (1.01 * E_lp + 4 * u) + tiny)
        labelled, beyond = y >= 0, y >= Cl
        pick = np.clip(y, 0, Cl - 1)
        a = np.take_along_axis(lp, pick[:, None, None].repeat(N, 1), -1)[..., 0]
        E_a0 = np.take_along_axis(E_lp, pick[:, None, None].repeat(N, 1), -1)[..., 0]
        a = np.where(beyond[:, None], np.nan, a)
        logp = np.where(labelled[:, None], a, 0.0)
        E_logp = np.where(labelled[:, None], E_a0, 0.0)
        w = np.ones(G) if cw is None else np.asarray(cw, np.float64)[pick]
        at = logp + lw
        E_at = E_logp + u * np.abs(np.where(np.isinf(at), 0.0, at))
        mx = at.max(-1)
        msafe = np.where(np.isinf(mx), 0.0, mx)
        ex = np.exp(at - msafe[:, None])
        sm = ex.sum(-1)
        lse = np.where(np.isinf(mx), mx, msafe + np.log(sm))
        logN = math.log(N)
        nll = np.where(labelled, -w * (lse - logN), 0.0)
        xent = np.where(labelled, -w * logp.mean(-1), 0.0)
        E_nll = np.where(labelled, np.abs(w) * (E_at.max(-1) + u * (2 * np.abs(msafe) + 11 * logN + Dn + 16)) + 2 * u * np.abs(nll), 0.0)
        E_xent = np.where(labelled, np.abs(w) / N * (E_logp.sum(-1) + (Dn + 2) * u * np.abs(logp).sum(-1)) + 2 * u * np.abs(xent), 0.0)
        pbar = p.mean(1)                                         # (G, Cl)
        E_probs = E_p.mean(1) + D2 * u * pbar
        h = -_xlogx(pbar)
        entropy = h.sum(-1)
        slope = np.where(pbar > 0, np.abs(np.log(np.where(pbar > 0, pbar, 1.0))) + 1.0, 0.0)
        E_entropy = (1.01 * slope * E_probs + 5 * u * np.abs(h)).sum(-1) + D3 * u * np.abs(h).sum(-1) + 1e-30
        plp = np.where(p == 0, 0.0, p * lp)
        alp = np.where(dead, 0.0, np.abs(lp))
        expent = -plp.sum(-1).mean(-1)
        E_expent = (E_p * (alp + 1) + p * E_lp + 2 * u * np.abs(plp)).sum(-1).mean(-1) + (D4 + 2) * u * np.abs(plp).sum(-1).mean(-1) + 1e-30
        out = dict(plan=pl, logp=logp, E_logp=E_logp, nll=nll, E_nll=E_nll, xent=xent, E_xent=E_xent,
                   probs=pbar[:, 1:] if binary else pbar, E_probs=E_probs[:, 1:] if binary else E_probs,
                   entropy=entropy, E_entropy=E_entropy, expected_entropy=expent, E_expected_entropy=E_expent,
                   mutual_information=np.where(np.isnan(entropy - expent), np.nan, np.maximum(entropy - expent, 0.0)),
                   E_mutual_information=E_entropy + E_expent)
        if grads is None:
            return out
        gn, gx, gl = (np.asarray(t, np.float64) for t in grads)
        r = ex / sm[:, None]
        R = np.expm1(2 * (E_at + u * np.abs(np.where(np.isinf(at), 0.0, at - msafe[:, None]))).max(-1)) + (Dn + 16) * u
        E_r = r * R[:, None] + tiny
        wg = (w * gn)[:, None]
        k = wg * r + (w * gx / N)[:, None] - gl
        k = np.where(beyond[:, None], np.nan, k)
        E_k = np.abs(wg) * E_r + 4 * u * (np.abs(wg) * r + np.abs(w * gx / N)[:, None] + np.abs(gl)) + tiny
        delta = (np.arange(Cl)[None, None, :] == y[:, None, None]).astype(np.float64)
        pd = p - delta
        gz = np.where(labelled[:, None, None], k[..., None] * pd, 0.0)
        E_gz = E_k[..., None] * np.abs(pd) + np.abs(k)[..., None] * (E_p + u * np.abs(pd)) + u * np.abs(gz) + tiny
        E_gz = np.where(labelled[:, None, None], E_gz, 0.0)
        glw = np.where(labelled[:, None], -wg * r, 0.0)
        glw = np.where(beyond[:, None], np.nan, glw)
        E_glw = np.where(labelled[:, None], np.abs(wg) * (E_r + 3 * u * r) + tiny, 0.0)
        if binary:
            gz, E_gz = gz[..., 1:], E_gz[..., 1:]
        out.update(grad_logits=gz, E_grad_logits=E_gz, grad_logw=glw, E_grad_logw=E_glw)
    return out


def worst(got, want, bound):
    """max over the elements of |got - want| / bound; elements where both are NaN, or the same infinity, agree (0); an element
    where one is NaN or infinite and the other is not is inf."""
    got, want, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64))
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & (got == want))
    odd = ~same & ~(np.isfinite(got) & np.isfinite(want))
    if odd.any():
        return float('inf')
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.where(same, 0.0, np.abs(got - want))
        ratio = np.where(err == 0, 0.0, err / np.where(same, 1.0, bound))
    return float(ratio.max()) if ratio.size else 0.0


# (groups G, pooled paths N, outer, stored width C; C = 0: binary).  tests/test_gpu_sample_class.py says why each is there.
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (3, 5, 2, 3), (2, 8, 1, 35), (2, 8, 1, 64), (2, 8, 1, 65), (1, 256, 1, 4), (2, 7, 1, 0),
          (9000, 2, 1, 2), (5, 2, 1, 35), (5, 3, 1, 35), (2, 4, 1, 32), (2, 4, 1, 33), (3, 8, 1, 10), (3, 9, 1, 10), (2, 128, 1, 2),
          (1, 64, 1, 4), (1, 65, 1, 4), (1, 3, 1, 256), (1, 3, 1, 257), (1, 96, 1, 256), (1, 96, 1, 257), (3, 1, 1, 0),
          (1, 256, 1, 0), (4100, 4, 1, 33), (1, 9, 1, 4099)]


def make_case(shape):
    """float32 inputs of a shape in the solve's layout - logits (outer, G N, C), labels (outer, G) int64 with group 0 unlabelled
    where G >= 2, logw (outer, G, N), class_weight, and upstream gradients - as a dict of numpy arrays."""
    G, N, O, C = shape
    binary = C == 0
    Cw, Cl = (1, 2) if binary else (C, C)
    rng = np.random.default_rng(G + 7 * N + 31 * O + 101 * C)
    z = (3.0 * rng.standard_normal((O, G, N, Cw))).astype(np.float32)
    y = rng.integers(0, Cl, (O, G)).astype(np.int64)
    if G >= 2:
        y[:, 0] = -1
    return dict(binary=binary, z=z.reshape(O, G * N, Cw), y=y, lw=(0.5 * rng.standard_normal((O, G, N))).astype(np.float32),
                cw=(0.5 + rng.random(Cl)).astype(np.float32), gn=rng.standard_normal((O, G)).astype(np.float32),
                gx=rng.standard_normal((O, G)).astype(np.float32), gl=rng.standard_normal((O, G, N)).astype(np.float32))


def case_reference(shape, case, with_weights, which='all', **kw):
    """`reference` of a `make_case` dict on the flattened groups (outer G); with_weights: logw and class_weight are used.
    which: the upstream gradients that arrive - 'nll', 'xent', 'logp' or 'all'."""
    G, N, O, C = shape
    f = lambda a, *s: np.asarray(a, np.float64).reshape(*s)
    zero = lambda a, on: a if on else np.zeros_like(a)
    grads = (zero(f(case['gn'], O * G), which in ('nll', 'all')), zero(f(case['gx'], O * G), which in ('xent', 'all')),
             zero(f(case['gl'], O * G, N), which in ('logp', 'all')))
    return reference(f(case['z'], O * G, N, -1), case['y'].reshape(O * G), f(case['lw'], O * G, N) if with_weights else None,
                     f(case['cw'], -1) if with_weights else None, case['binary'], grads, **kw)
