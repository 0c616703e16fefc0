"""Exact-rational known answers for the two spline coefficient constructions -> tests/golden/spline_exact.npz.

Everything here is `fractions.Fraction` arithmetic on float32-representable inputs, computed from the DEFINITIONS of the two
constructions and asserted against those definitions before anything is written.  Nothing is imported from oracle/, from the
package or from the reference: a transcription slip in a closed form cannot pass, because no closed form is typed in.

Stored form of one interval [t_j, t_j+1]:  [a, b, two_c, three_d]  with  p(s) = a + b s + two_c s^2 / 2 + three_d s^3 / 3,
s = t - t_j.

Fill (Hermite only).  An interior missing value is the linear interpolant in time between the nearest observed neighbours;
leading missing values take the first observation, trailing ones the last; a series without an observation is all zeros.

Hermite cubic with backward differences.  On interval k of width h the unique cubic with
    p(0) = x_k,   p(h) = x_k+1,   p'(0) = m_k-1  (m_0 on the first interval),   p'(h) = m_k,     m_k = (x_k+1 - x_k) / h_k.
The four conditions are solved as a 4 x 4 rational system and asserted on the result.

Natural cubic spline (the reference's controldiffeq/interpolate.py:84-150).  The knots are the observed entries together with both
ends, a missing end imputed with the first / last observation.  Through those knots: the C2 piecewise cubic that interpolates
them with zero second derivative at both ends.  Each piece is the cubic fixed by its two end values and two end derivatives (a
4 x 4 system again); the knot derivatives are the solution of the dense system "second derivatives agree at interior knots, vanish
at the ends".  Two knots give the straight line, no observation gives zeros.  Every original interval j gets the Taylor
re-expansion at t_j of the piece that contains it.  Asserted on the STORED coefficients: interpolation at every knot, C1 and C2 at
every original time, C3 at the original times that are no knots, zero curvature at both ends, and polynomial identity between
each re-expanded piece and its parent.

Per case (one `times` vector, S series):
    times (L,) float32;  X (S, L) float32, NaN = missing;  names (S,) str
    natural, hermite              (S, L-1, 4) float64, one rounding from the rational
    zero_natural, zero_hermite    (S, L-1, 4) bool: 0 in exact arithmetic AND exactly 0.0 in any correct float32 construction
        natural: two_c, three_d of a two-knot series (the straight line is a branch, not a solve); b, two_c, three_d for one
                 observation (every knot difference is x - x); everything without an observation
        hermite: two_c, three_d on the first interval (its entering slope IS m_0); b, two_c, three_d where m_k and the entering
                 slope both come from equal filled values (leading / trailing runs, one observation); everything without an
                 observation.  NOT the interior of a linearly filled gap: float32 leaves round-off there.
    hermite_bit_exact (S,) bool: every intermediate of the float32 formula (fill weight and product, x1 - x0, m, m - b, the
        quotients) is a float32 value, so a correct float32 construction returns the float32 image of the rational bit for bit.
        Decided by checking each intermediate, not by tag; the generator asserts that the dyadic series come out True.

Run from the repo root:  python tests/golden/make_spline_exact_golden.py     (needs numpy only)
"""
import io
import os
import random
import struct
import zipfile
from fractions import Fraction as Fr

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = 'spline_exact.npz'


def f32(x):
    """Nearest float32 of a python float / Fraction, as a Fraction."""
    return Fr(struct.unpack('f', struct.pack('f', float(x)))[0])


def is_f32(x):
    return f32(x) == x


# ---- linear algebra over the rationals --------------------------------------------------------------------------------------

def solve(A, rhs):
    """Gauss-Jordan with Fractions: the unique x with A x = rhs (asserts that A is regular and that the result solves it)."""
    n = len(A)
    M = [list(map(Fr, A[i])) + [Fr(rhs[i])] for i in range(n)]
    for col in range(n):
        piv = next((r for r in range(col, n) if M[r][col] != 0), None)
        assert piv is not None, 'singular system'
        M[col], M[piv] = M[piv], M[col]
        inv = 1 / M[col][col]
        M[col] = [v * inv for v in M[col]]
        for r in range(n):
            if r != col and M[r][col] != 0:
                f = M[r][col]
                M[r] = [v - f * w for v, w in zip(M[r], M[col])]
    x = [M[i][n] for i in range(n)]
    for i in range(n):
        assert sum(Fr(A[i][j]) * x[j] for j in range(n)) == rhs[i]
    return x


# stored form [a, b, two_c, three_d]: value and derivatives at offset s
def val(q, s):
    return q[0] + q[1] * s + q[2] * s * s / 2 + q[3] * s * s * s / 3


def d1(q, s):
    return q[1] + q[2] * s + q[3] * s * s


def d2(q, s):
    return q[2] + 2 * q[3] * s


def d3(q, s):
    return 2 * q[3]


def cubic_from_end_conditions(h, v0, v1, s0, s1):
    """The stored-form cubic with p(0) = v0, p(h) = v1, p'(0) = s0, p'(h) = s1: the four conditions as a 4 x 4 system."""
    A = [[1, 0, 0, 0],
         [1, h, h * h / 2, h * h * h / 3],
         [0, 1, 0, 0],
         [0, 1, h, h * h]]
    q = solve(A, [v0, v1, s0, s1])
    assert val(q, 0) == v0 and val(q, h) == v1 and d1(q, 0) == s0 and d1(q, h) == s1
    return q


# ---- fill -------------------------------------------------------------------------------------------------------------------

def fill(t, x):
    """x: list of Fraction or None (missing)."""
    L = len(x)
    obs = [j for j in range(L) if x[j] is not None]
    if not obs:
        return [Fr(0)] * L
    out = []
    for j in range(L):
        if x[j] is not None:
            out.append(x[j])
            continue
        prev = [i for i in obs if i < j]
        nxt = [i for i in obs if i > j]
        if not prev:
            out.append(x[nxt[0]])
        elif not nxt:
            out.append(x[prev[-1]])
        else:
            p, n = prev[-1], nxt[0]
            out.append(x[p] + (t[j] - t[p]) / (t[n] - t[p]) * (x[n] - x[p]))
    # the definition, asserted: observed entries kept; ends constant; interior collinear with its observed neighbours
    for j in range(L):
        if x[j] is not None:
            assert out[j] == x[j]
        elif j < obs[0]:
            assert out[j] == x[obs[0]]
        elif j > obs[-1]:
            assert out[j] == x[obs[-1]]
        else:
            p, n = max(i for i in obs if i < j), min(i for i in obs if i > j)
            assert (out[j] - x[p]) * (t[n] - t[p]) == (x[n] - x[p]) * (t[j] - t[p])
    return out


# ---- Hermite ----------------------------------------------------------------------------------------------------------------

def hermite(t, x):
    xf = fill(t, x)
    L = len(t)
    m = [(xf[k + 1] - xf[k]) / (t[k + 1] - t[k]) for k in range(L - 1)]
    out = []
    for k in range(L - 1):
        h = t[k + 1] - t[k]
        enter = m[k - 1] if k > 0 else m[0]
        q = cubic_from_end_conditions(h, xf[k], xf[k + 1], enter, m[k])
        out.append(q)
    # C1 across the grid: the leaving slope of interval k is the entering slope of interval k + 1
    for k in range(L - 2):
        h = t[k + 1] - t[k]
        assert val(out[k], h) == out[k + 1][0] and d1(out[k], h) == out[k + 1][1]
    return out


def hermite_zero_mask(x):
    """b, two_c, three_d where m_k and the entering slope both come from EQUAL FILLED values: interval k is flat by fill when k and
    k + 1 both lie in the leading run (first observation included) or both in the trailing run (last observation included)."""
    L = len(x)
    obs = [j for j in range(L) if x[j] is not None]
    mask = [[False] * 4 for _ in range(L - 1)]
    if not obs:
        return [[True] * 4 for _ in range(L - 1)]
    flat = [(k + 1 <= obs[0]) or (k >= obs[-1]) for k in range(L - 1)]
    for k in range(L - 1):
        if flat[k] and (flat[k - 1] if k > 0 else True):
            mask[k][1] = mask[k][2] = mask[k][3] = True
    mask[0][2] = mask[0][3] = True          # b_0 = m_0: m_0 - b_0 is x - x
    return mask


def hermite_float32_is_exact(t, x):
    """True when every intermediate of the float32 formula is a float32 value (then no operation rounds)."""
    L = len(x)
    obs = [j for j in range(L) if x[j] is not None]
    steps = []
    xf = fill(t, x)
    for j in range(L):
        if x[j] is None and obs and obs[0] < j < obs[-1]:
            p, n = max(i for i in obs if i < j), min(i for i in obs if i > j)
            w = (t[j] - t[p]) / (t[n] - t[p])
            steps += [t[j] - t[p], t[n] - t[p], w, x[n] - x[p], w * (x[n] - x[p]), x[p] + w * (x[n] - x[p])]
    prev = None
    for k in range(L - 1):
        h = t[k + 1] - t[k]
        dx = xf[k + 1] - xf[k]
        m = dx / h
        b = m if k == 0 else prev
        steps += [h, dx, m, m - b, 4 * (m - b), 4 * (m - b) / h, -3 * (m - b), h * h, -3 * (m - b) / (h * h)]
        prev = m
    return all(is_f32(s) for s in steps)


# ---- natural ----------------------------------------------------------------------------------------------------------------

def natural_knots(t, x):
    """(indices, values) of the knots: observed entries and both ends, a missing end imputed; None without an observation."""
    L = len(x)
    obs = [j for j in range(L) if x[j] is not None]
    if not obs:
        return None
    idx = sorted(set(obs) | {0, L - 1})
    vals = []
    for j in idx:
        if x[j] is not None:
            vals.append(x[j])
        else:
            vals.append(x[obs[0]] if j == 0 else x[obs[-1]])
    return idx, vals


def natural(t, x):
    L = len(t)
    kn = natural_knots(t, x)
    if kn is None:
        return [[Fr(0)] * 4 for _ in range(L - 1)]
    idx, y = kn
    T = [t[j] for j in idx]
    n = len(idx)
    H = [T[i + 1] - T[i] for i in range(n - 1)]
    # piece i as a linear function of the knot derivatives: q_i = base_i + k_i * e0_i + k_i+1 * e1_i
    base = [cubic_from_end_conditions(H[i], y[i], y[i + 1], Fr(0), Fr(0)) for i in range(n - 1)]
    e0 = [cubic_from_end_conditions(H[i], Fr(0), Fr(0), Fr(1), Fr(0)) for i in range(n - 1)]
    e1 = [cubic_from_end_conditions(H[i], Fr(0), Fr(0), Fr(0), Fr(1)) for i in range(n - 1)]
    # dense system in the n knot derivatives: zero curvature at both ends, equal curvature from both sides at interior knots
    A = [[Fr(0)] * n for _ in range(n)]
    r = [Fr(0)] * n
    A[0][0], A[0][1], r[0] = d2(e0[0], 0), d2(e1[0], 0), -d2(base[0], 0)
    A[n - 1][n - 2], A[n - 1][n - 1], r[n - 1] = d2(e0[n - 2], H[n - 2]), d2(e1[n - 2], H[n - 2]), -d2(base[n - 2], H[n - 2])
    for i in range(1, n - 1):
        A[i][i - 1] += d2(e0[i - 1], H[i - 1])
        A[i][i] += d2(e1[i - 1], H[i - 1]) - d2(e0[i], 0)
        A[i][i + 1] -= d2(e1[i], 0)
        r[i] = d2(base[i], 0) - d2(base[i - 1], H[i - 1])
    k = solve(A, r)
    piece = [[base[i][c] + k[i] * e0[i][c] + k[i + 1] * e1[i][c] for c in range(4)] for i in range(n - 1)]
    if n == 2:      # exactly two knots: the straight line
        assert piece[0][2] == 0 and piece[0][3] == 0 and piece[0][1] == (y[1] - y[0]) / H[0]
    # Taylor re-expansion of the containing piece at every original time
    out, parent = [], []
    for j in range(L - 1):
        i = max(i for i in range(n - 1) if T[i] <= t[j])
        assert T[i] <= t[j] < T[i + 1]
        s = t[j] - T[i]
        q = [val(piece[i], s), d1(piece[i], s), d2(piece[i], s), d3(piece[i], s) / 2]
        out.append(q)
        parent.append(i)
        for u in (Fr(0), Fr(1, 3), Fr(-1, 2), Fr(2), Fr(-5, 7)):     # five points fix a cubic: same polynomial as the parent
            assert val(q, u) == val(piece[i], s + u)
    # the definition, asserted on the stored coefficients
    for i, j in enumerate(idx):                                       # interpolation at every knot
        if j < L - 1:
            assert out[j][0] == y[i]
        else:
            assert val(out[L - 2], t[L - 1] - t[L - 2]) == y[i]
    for j in range(L - 2):                                            # C2 everywhere, C3 where no knot sits
        h = t[j + 1] - t[j]
        assert val(out[j], h) == out[j + 1][0]
        assert d1(out[j], h) == out[j + 1][1]
        assert d2(out[j], h) == out[j + 1][2]
        if (j + 1) not in idx:
            assert out[j][3] == out[j + 1][3] and parent[j] == parent[j + 1]
    assert out[0][2] == 0 and d2(out[L - 2], t[L - 1] - t[L - 2]) == 0   # natural ends
    return out


def natural_zero_mask(x):
    L = len(x)
    obs = [j for j in range(L) if x[j] is not None]
    if not obs:
        return [[True] * 4 for _ in range(L - 1)]
    knots = len(set(obs) | {0, L - 1})
    row = [False, len(obs) == 1, knots == 2 or len(obs) == 1, knots == 2 or len(obs) == 1]
    return [list(row) for _ in range(L - 1)]


# ---- cases ------------------------------------------------------------------------------------------------------------------

def irregular_times(rng, L, lo=0.25, hi=2.0, small_gap_at=None):
    t = [Fr(0)]
    for k in range(L - 1):
        gap = f32(rng.uniform(0.1, 0.3) if k == small_gap_at else rng.uniform(lo, hi))
        t.append(f32(t[-1] + gap))
    return t


def normals(rng, L):
    return [f32(rng.gauss(0.0, 1.0)) for _ in range(L)]


def dyadic_values(rng, L):
    return [Fr(rng.randint(-32, 32), 8) for _ in range(L)]


def masked(vals, missing):
    return [None if j in missing else v for j, v in enumerate(vals)]


def only(vals, keep):
    return [v if j in keep else None for j, v in enumerate(vals)]


def build_cases():
    rng = random.Random(20240607)
    cases = {}
    # dyadic: every float32 intermediate of the Hermite formula is representable
    L = 9
    grids = {'dyadic_unit': [Fr(k) for k in range(L)],
             'dyadic_pow2': [sum([Fr(1, 2), Fr(1, 2), Fr(1, 4), Fr(1, 4), Fr(1, 4), Fr(1, 4), Fr(2), Fr(1)][:k], Fr(0)) for k in range(L)]}
    for tag, t in grids.items():
        series = []
        for r in range(3):
            series.append((f'no NaN #{r}', dyadic_values(rng, L)))
        series.append(('run of 1 (weight 1/2)', masked(dyadic_values(rng, L), {1})))
        series.append(('run of 3 (weights 1/4, 1/2, 3/4)', masked(dyadic_values(rng, L), {3, 4, 5})))
        series.append(('runs of 1 and 3', masked(dyadic_values(rng, L), {1, 3, 4, 5})))
        cases[tag] = (t, series)
    # irregular
    L = 12
    t = irregular_times(rng, L)
    series = [(f'no NaN #{r}', normals(rng, L)) for r in range(4)]
    for r in range(6):
        series.append((f'40% NaN #{r}', masked(normals(rng, L), {j for j in range(L) if rng.random() < 0.4})))
    cases['irregular'] = (t, series)
    # edges
    L = 9
    t = irregular_times(rng, L)
    pats = [('interior-only run', masked, {3, 4, 5}),
            ('leading run', masked, {0, 1, 2}),
            ('trailing run', masked, {6, 7, 8}),
            ('both ends missing', masked, {0, 8}),
            ('runs at both ends and inside', masked, {0, 1, 4, 7, 8}),
            ('one observation at 0', only, {0}),
            ('one observation at L-1', only, {L - 1}),
            ('one observation, interior', only, {4}),
            ('two observations, adjacent', only, {3, 4}),
            ('two observations, ends only', only, {0, L - 1}),
            ('two observations, interior only', only, {2, 6}),
            ('no observation', only, set())]
    cases['edges'] = (t, [(name, fn(normals(rng, L), idx)) for name, fn, idx in pats])
    # short
    t = [Fr(0), f32(0.2704)]
    cases['short2'] = (t, [(name, masked(normals(rng, 2), miss)) for name, miss in
                           (('none missing', set()), ('first missing', {0}), ('last missing', {1}), ('both missing', {0, 1}))])
    t = irregular_times(rng, 3, small_gap_at=1)
    cases['short3'] = (t, [('observed ' + ''.join(str((mk >> j) & 1) for j in range(3)),
                            only(normals(rng, 3), {j for j in range(3) if (mk >> j) & 1})) for mk in range(8)])
    return cases


def to_f64(x):
    return np.array([[[float(v) for v in q] for q in s] for s in x], dtype=np.float64)


def generate():
    out = {}
    cases = build_cases()
    for tag, (t, series) in cases.items():
        L = len(t)
        assert 2 <= L <= 12 and all(is_f32(v) for v in t) and all(t[j + 1] > t[j] for j in range(L - 1))
        if tag.startswith('short'):
            assert min(t[j + 1] - t[j] for j in range(L - 1)) < Fr(3, 10)
        for _, x in series:
            assert all(v is None or is_f32(v) for v in x)
        nat = [natural(t, x) for _, x in series]
        her = [hermite(t, x) for _, x in series]
        zn = np.array([natural_zero_mask(x) for _, x in series], dtype=bool)
        zh = np.array([hermite_zero_mask(x) for _, x in series], dtype=bool)
        exact = np.array([hermite_float32_is_exact(t, x) for _, x in series], dtype=bool)
        for s in range(len(series)):                        # what is marked zero IS zero
            for j in range(L - 1):
                for c in range(4):
                    assert not zn[s, j, c] or nat[s][j][c] == 0, (tag, s, j, c)
                    assert not zh[s, j, c] or her[s][j][c] == 0, (tag, s, j, c)
        if tag.startswith('dyadic'):
            assert exact.all(), (tag, exact)
        out[f'{tag}/times'] = np.array([float(v) for v in t], dtype=np.float32)
        out[f'{tag}/X'] = np.array([[np.nan if v is None else float(v) for v in x] for _, x in series], dtype=np.float32)
        out[f'{tag}/names'] = np.array([name for name, _ in series])
        out[f'{tag}/natural'] = to_f64(nat)
        out[f'{tag}/hermite'] = to_f64(her)
        out[f'{tag}/zero_natural'] = zn
        out[f'{tag}/zero_hermite'] = zh
        out[f'{tag}/hermite_bit_exact'] = exact
        print(f'  {tag}: L = {L}, {len(series)} series, {int(exact.sum())} Hermite bit-exact', flush=True)
    out['meta/cases'] = np.array(list(cases))
    return out


def write(path, arrays):
    """An .npz with fixed member timestamps and stored (uncompressed) members, so that the same arrays give the same file whatever
    the zlib at hand."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_STORED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(directory=HERE):
    arrays = generate()
    path = os.path.join(directory, FIXTURE)
    write(path, arrays)
    print('wrote', path, f'{os.path.getsize(path)} bytes, {len(arrays)} arrays')
    return path


if __name__ == '__main__':
    main()
