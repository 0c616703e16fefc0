// Spline coefficient construction on the GPU: the reference builds these offline with
// Python loops over batch x channel x time (controldiffeq/interpolate.py:9-155, minutes on real datasets).
// One thread owns one scalar series (batch row b, channel c) and runs the sequential parts (Thomas solve over the
// OBSERVED knots, re-expansion onto every original sub-interval) with the reference's operation order and no FMA
// contraction; per-series temporaries live in a [L][series] workspace so neighbouring threads stay coalesced.
#include "snsde_internal.h"

namespace {

struct SplineArgs {
    const float* times;   // (L)
    const float* X;       // (B, L, C), NaN = missing
    float* out;           // (B, L-1, 4C) = cat[a, b, two_c, three_d]
    int32_t* oidx;        // workspace [L][S]
    float* nd;            // workspace [L][S]
    float* nb;            // workspace [L][S]
    float* kd;            // workspace [L][S]
    int32_t B, L, C;
};

__global__ void snsde_natural_spline_kernel(SplineArgs a) {
#pragma clang fp contract(off)
    const int S = a.B * a.C, L = a.L, C = a.C;
    const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= S) return;
    const int b = sidx / C, c = sidx - b * C;
    const float* x = a.X + (size_t)b * L * C + c;          // x[j * C]
    float* out = a.out + (size_t)b * (L - 1) * 4 * C + c;  // out[j * 4C + k * C]
    // ---- observed knots; the ends are imputed with the first / last observation (interpolate.py:100-114)
    int first = -1, last = -1;
    for (int j = 0; j < L; ++j) {
        const float v = x[(size_t)j * C];
        if (v == v) { if (first < 0) first = j; last = j; }
    }
    if (first < 0) {   // every entry missing: zero coefficients (interpolate.py:84-92)
        for (int j = 0; j < L - 1; ++j)
            for (int k = 0; k < 4; ++k) out[(size_t)j * 4 * C + k * C] = 0.0f;
        return;
    }
    const float xfirst = x[(size_t)first * C], xlast = x[(size_t)last * C];
    int m = 0;
    for (int j = 0; j < L; ++j) {
        const float v = x[(size_t)j * C];
        if (v == v || j == 0 || j == L - 1) { a.oidx[(size_t)m * S + sidx] = j; ++m; }
    }
    auto tc = [&](int i) { return a.times[a.oidx[(size_t)i * S + sidx]]; };
    auto xc = [&](int i) {
        const int j = a.oidx[(size_t)i * S + sidx];
        const float v = x[(size_t)j * C];
        return (v == v) ? v : (j == 0 ? xfirst : xlast);
    };
    // ---- knot derivatives of the natural spline through the m observed knots (interpolate.py:9-55, misc.py:12-66)
    if (m > 2) {
        float rec_prev = 0.0f, sc_prev = 0.0f, ndp = 0.0f, nbp = 0.0f;
        for (int i = 0; i < m; ++i) {
            float rec = 0.0f, sc = 0.0f;
            if (i < m - 1) {
                rec = 1.0f / (tc(i + 1) - tc(i));
                sc = (3.0f * (xc(i + 1) - xc(i))) * (rec * rec);
            }
            float diag, rhs;
            if (i == 0) { diag = rec; rhs = sc; }
            else if (i == m - 1) { diag = 0.0f + rec_prev; rhs = 0.0f + sc_prev; }
            else { diag = rec + rec_prev; rhs = sc + sc_prev; }
            diag = diag * 2.0f;
            float ndv, nbv;
            if (i == 0) { ndv = diag; nbv = rhs; }
            else {
                const float w = rec_prev / ndp;
                ndv = diag - w * rec_prev;
                nbv = rhs - w * nbp;
            }
            a.nd[(size_t)i * S + sidx] = ndv;
            a.nb[(size_t)i * S + sidx] = nbv;
            ndp = ndv; nbp = nbv; rec_prev = rec; sc_prev = sc;
        }
        float kn = nbp / ndp;
        a.kd[(size_t)(m - 1) * S + sidx] = kn;
        for (int i = m - 2; i >= 0; --i) {
            const float rec = 1.0f / (tc(i + 1) - tc(i));
            kn = (a.nb[(size_t)i * S + sidx] - rec * kn) / a.nd[(size_t)i * S + sidx];
            a.kd[(size_t)i * S + sidx] = kn;
        }
    }
    // ---- coefficients on every original interval (interpolate.py:116-150)
    int p = -1;
    float A = 0.f, Bc = 0.f, C2 = 0.f, D3 = 0.f, tprev = 0.f;
    for (int j = 0; j < L - 1; ++j) {
        const float tj = a.times[j];
        if (p + 1 < m - 1 && tj >= tc(p + 1)) {
            ++p;
            tprev = tc(p);
            const float x0 = xc(p), x1 = xc(p + 1);
            if (m == 2) {
                A = x0; Bc = (x1 - x0) / (tc(1) - tc(0)); C2 = 0.0f; D3 = 0.0f;
            } else {
                const float rec = 1.0f / (tc(p + 1) - tprev);
                const float six = 2.0f * (3.0f * (x1 - x0));
                const float k0 = a.kd[(size_t)p * S + sidx], k1 = a.kd[(size_t)(p + 1) * S + sidx];
                A = x0; Bc = k0;
                C2 = (six * rec - 4.0f * k0 - 2.0f * k1) * rec;
                D3 = (-six * rec + 3.0f * (k0 + k1)) * (rec * rec);
            }
        }
        const float off = tprev - tj;
        const float a_inner = (0.5f * C2 - D3 * off / 3.0f) * off;
        out[(size_t)j * 4 * C] = A + (a_inner - Bc) * off;
        out[(size_t)j * 4 * C + C] = Bc + (D3 * off - C2) * off;
        out[(size_t)j * 4 * C + 2 * C] = C2 - 2.0f * D3 * off;
        out[(size_t)j * 4 * C + 3 * C] = D3;
    }
}

// torchcde hermite_cubic_coefficients_with_backward_differences: missing values filled linearly in
// time between observed neighbours (ends: nearest observation; all-missing: 0), then per interval
// a = x_k, b = previous secant slope (own slope on the first interval), two_c = 4 (m_k - b)/h, three_d = -3 (m_k - b)/h^2.
__global__ void snsde_hermite_kernel(const float* __restrict__ times, const float* __restrict__ X, float* __restrict__ outp,
                                     int B, int L, int C) {
#pragma clang fp contract(off)
    const int S = B * C;
    const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= S) return;
    const int b = sidx / C, c = sidx - b * C;
    const float* x = X + (size_t)b * L * C + c;
    float* out = outp + (size_t)b * (L - 1) * 4 * C + c;
    int first = -1;
    for (int j = 0; j < L && first < 0; ++j) { const float v = x[(size_t)j * C]; if (v == v) first = j; }
    // filled value at position j given the previous observed (pj, pv) and the next observed found by scanning
    int pj = -1; float pv = 0.0f;
    int nj = first; float nv = first >= 0 ? x[(size_t)first * C] : 0.0f;
    auto filled = [&](int j) {
        if (first < 0) return 0.0f;
        const float v = x[(size_t)j * C];
        if (v == v) { pj = j; pv = v; return v; }
        if (nj >= 0 && nj < j) { nj = -1; }
        if (nj < 0 || nj <= j) {      // find the next observation after j
            nj = -1;
            for (int q = j + 1; q < L; ++q) { const float w = x[(size_t)q * C]; if (w == w) { nj = q; nv = w; break; } }
            if (nj < 0) nj = L;       // none
        }
        if (pj < 0) return nv;        // leading gap
        if (nj >= L) return pv;       // trailing gap
        const float wgt = (times[j] - times[pj]) / (times[nj] - times[pj]);
        return pv + wgt * (nv - pv);
    };
    float x0 = filled(0), mprev = 0.0f;
    for (int j = 0; j < L - 1; ++j) {
        const float x1 = filled(j + 1);
        const float h = times[j + 1] - times[j];
        const float mk = (x1 - x0) / h;
        const float bb = (j == 0) ? mk : mprev;
        out[(size_t)j * 4 * C] = x0;
        out[(size_t)j * 4 * C + C] = bb;
        out[(size_t)j * 4 * C + 2 * C] = 4.0f * (mk - bb) / h;
        out[(size_t)j * 4 * C + 3 * C] = -3.0f * (mk - bb) / (h * h);
        mprev = mk; x0 = x1;
    }
}

// ---- adjoints of the two constructions: grad_coeffs (B, L-1, 4C) -> grad_X (B, L, C) ------------------------------------------
// Both maps are linear in the observed values; the knot compaction, the matrix, the end imputation and the offsets depend on
// `times` and on WHICH entries are NaN only.  So the adjoint is the transpose, X is read for its mask, and nothing of the forward
// is kept.  One lane owns one series and writes every entry of its grad_X column exactly once (missing entries: 0.0f); no
// atomics, no cross-lane step, a fixed operation order (no FMA contraction): bit-equal from run to run and from batch to batch.

struct SplineBwdArgs {
    const float* times;   // (L)
    const float* X;       // (B, L, C): the NaN mask
    const float* g;       // (B, L-1, 4C) cotangent of cat[a, b, two_c, three_d]
    float* gx;            // (B, L, C) out
    float* nd;            // workspace [L][S]: pivots of the forward elimination (they depend on rec only)
    float* nb;            // workspace [L][S]: eliminated right-hand side gk
    float* gdx;           // workspace [L][S]: direct part of the cotangent of dx_p (through C2 and D3)
    float* ga;            // workspace [L][S]: cotangent of A_p = xc_p
    int32_t B, L, C;
};

// Transpose of snsde_natural_spline_kernel.  With k = T^-1 rhs, T symmetric tridiagonal (diag_i = 2 (rec_{i-1} + rec_i), off-diagonal
// rec_i), rhs_i = sc_{i-1} + sc_i, sc_i = 3 dx_i rec_i^2:
//   ascending sweep  : per compressed interval p, (gA, gBc, gC2, gD3) = polynomial-weighted sums of the cotangents of its original
//                      intervals j (ascending j); gk_p is complete once interval p is closed, so the forward elimination of
//                      T u = gk runs in the same sweep with the pivots rebuilt from rec;
//   descending sweep : back substitution, g sc_i = u_i + u_{i+1}, g dx_i = direct + 3 rec_i^2 g sc_i,
//                      g xc_i = gA_i + g dx_{i-1} - g dx_i, scattered to the observed entries; an imputed end hands its cotangent
//                      to the first / last observation.
__global__ void snsde_natural_spline_backward_kernel(SplineBwdArgs a) {
#pragma clang fp contract(off)
    const int S = a.B * a.C, L = a.L, C = a.C;
    const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= S) return;
    const int b = sidx / C, c = sidx - b * C;
    const float* x = a.X + (size_t)b * L * C + c;             // x[j * C]
    const float* g = a.g + (size_t)b * (L - 1) * 4 * C + c;   // g[j * 4C + k * C]
    float* gx = a.gx + (size_t)b * L * C + c;
    auto observed = [&](int j) { const float v = x[(size_t)j * C]; return v == v; };
    // ---- ascending sweep
    int first = -1, last = -1, p = 0;
    float tprev = a.times[0];
    float gA = 0.f, gBc = 0.f, gC2 = 0.f, gD3 = 0.f;
    float gk = 0.f, rec_prev = 0.f, ndp = 0.f, nbp = 0.f;
    for (int j = 0; j < L; ++j) {
        const bool obs = observed(j);
        if (obs) { if (first < 0) first = j; last = j; }
        const float tj = a.times[j];
        if (j > 0 && (obs || j == L - 1)) {      // knot p + 1: close compressed interval p
            if (p == 0 && j == L - 1) break;     // m == 2: (gA, gBc) are all there is
            const float rec = 1.0f / (tj - tprev);
            const float rr = rec * rec;
            const float gkp = gk + ((gBc - 4.0f * rec * gC2) + 3.0f * rr * gD3);
            const float diag = (rec + rec_prev) * 2.0f;
            float ndv, nbv;
            if (p == 0) { ndv = diag; nbv = gkp; }
            else {
                const float w = rec_prev / ndp;
                ndv = diag - w * rec_prev;
                nbv = gkp - w * nbp;
            }
            a.nd[(size_t)p * S + sidx] = ndv;
            a.nb[(size_t)p * S + sidx] = nbv;
            a.gdx[(size_t)p * S + sidx] = (6.0f * (gC2 - gD3 * rec)) * rr;
            a.ga[(size_t)p * S + sidx] = gA;
            gk = 3.0f * rr * gD3 - 2.0f * rec * gC2;
            ndp = ndv; nbp = nbv; rec_prev = rec;
            ++p; tprev = tj;
            gA = 0.f; gBc = 0.f; gC2 = 0.f; gD3 = 0.f;
        }
        if (j < L - 1) {
            const float off = tprev - tj;
            const float ga = g[(size_t)j * 4 * C], gb = g[(size_t)j * 4 * C + C];
            const float gc = g[(size_t)j * 4 * C + 2 * C], gd = g[(size_t)j * 4 * C + 3 * C];
            gA = gA + ga;
            gBc = gBc + (gb - ga * off);
            gC2 = gC2 + ((0.5f * ga * off - gb) * off + gc);
            gD3 = gD3 + (((gb - ga * off / 3.0f) * off - 2.0f * gc) * off + gd);
        }
    }
    if (first < 0) {                             // no observation: the coefficients are constants
        for (int j = 0; j < L; ++j) gx[(size_t)j * C] = 0.0f;
        return;
    }
    const bool obs0 = first == 0, obsL = last == L - 1;
    if (p == 0) {                                // m == 2: A = x0, Bc = (x1 - x0) / (t_{L-1} - t_0); at least one end is observed
        const float gdx = gBc / (a.times[L - 1] - a.times[0]);
        const float g0 = gA - gdx, g1 = gdx;
        for (int j = 1; j < L - 1; ++j) gx[(size_t)j * C] = 0.0f;
        gx[0] = obs0 ? (obsL ? g0 : g0 + g1) : 0.0f;
        gx[(size_t)(L - 1) * C] = obsL ? (obs0 ? g1 : g1 + g0) : 0.0f;
        return;
    }
    // ---- descending sweep; p = m - 1 compressed intervals were closed, the last row of the elimination is row p
    float u_next;
    {
        const float w = rec_prev / ndp;
        u_next = (gk - w * nbp) / (rec_prev * 2.0f - w * rec_prev);
    }
    int jn = L - 1;                              // the knot to the right, its cotangent still lacks g dx of the interval to its left
    float gA_n = 0.0f, gdx_right = 0.0f;
    float carry_last = 0.0f, gfirst = 0.0f;
    auto emit = [&](int j, float v) {            // cotangent of compressed value at knot j
        const bool o = (j == 0) ? obs0 : ((j == L - 1) ? obsL : true);
        if (!o) {                                // imputed end
            if (j == 0) { gfirst = gfirst + v; } else { carry_last = v; }
            gx[(size_t)j * C] = 0.0f;
            return;
        }
        if (j == last && !obsL) v = v + carry_last;
        if (j == first) gfirst = v; else gx[(size_t)j * C] = v;
    };
    int i = p - 1;
    for (int j = L - 2; j >= 0; --j) {
        if (j == 0 || observed(j)) {
            const float rec = 1.0f / (a.times[jn] - a.times[j]);
            const float u = (a.nb[(size_t)i * S + sidx] - rec * u_next) / a.nd[(size_t)i * S + sidx];
            const float gdx = a.gdx[(size_t)i * S + sidx] + (3.0f * (u + u_next)) * (rec * rec);
            emit(jn, (gA_n + gdx) - gdx_right);
            gA_n = a.ga[(size_t)i * S + sidx];
            gdx_right = gdx; u_next = u; jn = j; --i;
        } else {
            gx[(size_t)j * C] = 0.0f;
        }
    }
    emit(0, gA_n - gdx_right);
    gx[(size_t)first * C] = gfirst;
}

// Transpose of snsde_hermite_kernel.  Descending j: g xf_j = ga_j + q_{j-1} - q_j with q_j = g m_j / h_j and
// g m_j = s_j + (gb_{j+1} - s_{j+1}), s_j = 4 gc_j / h_j - 3 gd_j / h_j^2 the cotangent of (m_j - b_j); on the first interval
// b_0 = m_0, so g m_0 = gb_0 + (gb_1 - s_1).  The linear fill is transposed in the same sweep: a missing j between observed
// pj < j < nj gives w g to nj and g - w g to pj (w the forward's weight), a leading gap everything to nj, a trailing gap
// everything to pj.
__global__ void snsde_hermite_backward_kernel(const float* __restrict__ times, const float* __restrict__ X,
                                              const float* __restrict__ gp, float* __restrict__ gxp, int B, int L, int C) {
#pragma clang fp contract(off)
    const int S = B * C;
    const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= S) return;
    const int b = sidx / C, c = sidx - b * C;
    const float* x = X + (size_t)b * L * C + c;
    const float* g = gp + (size_t)b * (L - 1) * 4 * C + c;
    float* gx = gxp + (size_t)b * L * C + c;
    auto observed = [&](int j) { const float v = x[(size_t)j * C]; return v == v; };
    float ga = 0.0f, gbs = 0.0f, q = 0.0f;       // of interval j: ga_j, gb_j - s_j, q_j (all 0 at j = L-1: there is no such interval)
    int nj = -1, pj = -2;                        // nj: observed entry to the right (-1: none); pj: cached previous observation (-2: unknown)
    float accn = 0.0f, accp = 0.0f;              // cotangents collected for nj and for the next observation to the left
    for (int j = L - 1; j >= 0; --j) {
        float gxf;
        if (j >= 1) {
            const size_t o = (size_t)(j - 1) * 4 * C;
            const float ga1 = g[o], gb1 = g[o + C], gc1 = g[o + 2 * C], gd1 = g[o + 3 * C];
            const float h = times[j] - times[j - 1];
            const float s1 = 4.0f * gc1 / h - 3.0f * gd1 / (h * h);
            const float gm = (j - 1 > 0 ? s1 : gb1) + gbs;
            const float q1 = gm / h;
            gxf = (ga + q1) - q;
            ga = ga1; gbs = gb1 - s1; q = q1;
        } else {
            gxf = ga - q;
        }
        if (observed(j)) {
            if (nj >= 0) gx[(size_t)nj * C] = accn;
            accn = gxf + accp; accp = 0.0f;
            nj = j; pj = -2;
            continue;
        }
        gx[(size_t)j * C] = 0.0f;
        if (nj < 0) { accp = accp + gxf; continue; }         // trailing gap
        if (pj == -2) {                                      // once per gap: the previous observation
            pj = -1;
            for (int r = j - 1; r >= 0; --r) if (observed(r)) { pj = r; break; }
        }
        if (pj < 0) { accn = accn + gxf; continue; }         // leading gap
        const float wgt = (times[j] - times[pj]) / (times[nj] - times[pj]);
        const float t = wgt * gxf;
        accn = accn + t;
        accp = accp + (gxf - t);
    }
    if (nj >= 0) gx[(size_t)nj * C] = accn;
}

}  // namespace

extern "C" {

size_t snsde_spline_workspace_bytes(int32_t batch, int32_t knots, int32_t channels) {
    if (batch <= 0 || knots < 2 || channels <= 0) return 0;
    return (size_t)4 * knots * batch * channels * sizeof(float) + 256;
}

int snsde_natural_cubic_coeffs(const float* times, const float* X, int32_t batch, int32_t knots, int32_t channels,
                               float* coeffs, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!times || !X || !coeffs || !workspace) return SNSDE_ERR_NULL;
    if (batch <= 0 || knots < 2 || channels <= 0) return SNSDE_ERR_DIMS;
    if (workspace_bytes < snsde_spline_workspace_bytes(batch, knots, channels)) return SNSDE_ERR_WORKSPACE;
    const size_t n = (size_t)knots * batch * channels;
    SplineArgs a;
    a.times = times; a.X = X; a.out = coeffs;
    a.oidx = static_cast<int32_t*>(workspace);
    a.nd = reinterpret_cast<float*>(a.oidx + n);
    a.nb = a.nd + n;
    a.kd = a.nb + n;
    a.B = batch; a.L = knots; a.C = channels;
    const int S = batch * channels;
    hipLaunchKernelGGL(snsde_natural_spline_kernel, dim3((S + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(hip_stream), a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

int snsde_hermite_coeffs(const float* times, const float* X, int32_t batch, int32_t knots, int32_t channels,
                         float* coeffs, void* hip_stream) {
    if (!times || !X || !coeffs) return SNSDE_ERR_NULL;
    if (batch <= 0 || knots < 2 || channels <= 0) return SNSDE_ERR_DIMS;
    const int S = batch * channels;
    hipLaunchKernelGGL(snsde_hermite_kernel, dim3((S + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(hip_stream),
                       times, X, coeffs, batch, knots, channels);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

size_t snsde_spline_backward_workspace_bytes(int32_t batch, int32_t knots, int32_t channels) {
    if (batch <= 0 || knots < 2 || channels <= 0) return 0;
    return (size_t)4 * knots * batch * channels * sizeof(float) + 256;
}

int snsde_natural_cubic_coeffs_backward(const float* times, const float* X, const float* grad_coeffs,
                                        int32_t batch, int32_t knots, int32_t channels,
                                        float* grad_X, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!times || !X || !grad_coeffs || !grad_X || !workspace) return SNSDE_ERR_NULL;
    if (batch <= 0 || knots < 2 || channels <= 0) return SNSDE_ERR_DIMS;
    if (workspace_bytes < snsde_spline_backward_workspace_bytes(batch, knots, channels)) return SNSDE_ERR_WORKSPACE;
    const size_t n = (size_t)knots * batch * channels;
    SplineBwdArgs a;
    a.times = times; a.X = X; a.g = grad_coeffs; a.gx = grad_X;
    a.nd = static_cast<float*>(workspace);
    a.nb = a.nd + n;
    a.gdx = a.nb + n;
    a.ga = a.gdx + n;
    a.B = batch; a.L = knots; a.C = channels;
    const int S = batch * channels;
    hipLaunchKernelGGL(snsde_natural_spline_backward_kernel, dim3((S + 127) / 128), dim3(128), 0,
                       static_cast<hipStream_t>(hip_stream), a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

int snsde_hermite_coeffs_backward(const float* times, const float* X, const float* grad_coeffs,
                                  int32_t batch, int32_t knots, int32_t channels, float* grad_X, void* hip_stream) {
    if (!times || !X || !grad_coeffs || !grad_X) return SNSDE_ERR_NULL;
    if (batch <= 0 || knots < 2 || channels <= 0) return SNSDE_ERR_DIMS;
    const int S = batch * channels;
    hipLaunchKernelGGL(snsde_hermite_backward_kernel, dim3((S + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(hip_stream),
                       times, X, grad_coeffs, grad_X, batch, knots, channels);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

}  // extern "C"

// ---- initial state from the control path (stand-alone form; the MFMA forward folds it into its prepare launch) ----
namespace {
__global__ void snsde_z0_kernel(SnsdeZ0Job z) { snsde_z0_rows(z, blockIdx.x, gridDim.x); }
}

int snsde_z0_launch(const snsde_solve* s, hipStream_t stream) {
    if (!s->z0_weight || !s->z0_bias || !s->y0 || !s->step_tab) return SNSDE_ERR_NULL;
    SnsdeZ0Job z{s->z0_weight, s->z0_bias, s->coeffs, s->step_tab, const_cast<float*>(s->y0), s->batch,
                 s->model.hidden_channels, s->model.input_channels, s->knots};
    const int total = s->batch * s->model.hidden_channels;
    int grid = (total + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(snsde_z0_kernel, dim3(grid), dim3(256), 0, stream, z);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

