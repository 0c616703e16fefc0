// Weighted sample sets: statistics, CRPS and quantiles of sample paths that carry log-weights, and their adjoints with the weights
// fixed (include/snsde.h: snsde_sample_stats_weighted, snsde_sample_crps_weighted, snsde_sample_quantiles_weighted and their
// _backward).  ys is (outer, M, G, S, W) as in snsde_scores.hip - the pooled set of an output element (o, g, w) is x_n, n = m S + s,
// N = M S <= 256 - and logw is (outer, G, N): one log-weight per pooled path, shared by the W columns of the group.
// Weights.  One wave normalises a group's weights on chip before any sample is read (normalise(), snsde_sample_set.h): lane l holds a_n for
// n = l, 64 + l, 128 + l, 192 + l (-Inf past N), mx by fmaxf, e_n = expf(a_n - mx), P and D' = sum w_n (1 - w_n) over one fixed
// 256-leaf tree (zeros past N), w_n = e_n / P.  w_n and a live mark (0, NaN where dead) go to two 1 KB LDS rows that every lane then reads by broadcast.
// A sample is dead where e_n == 0 and P is a number: it is selected out by a branch that is uniform over the workgroup, never
// multiplied, so whatever it holds reaches nothing.  In a group whose P is NaN (all -Inf, a NaN or a +Inf weight) every w_n is NaN,
// 0 / NaN included, nothing is selected out and NaN reaches every output of the group by the arithmetic.
// Ownership.  The score kernels keep the tiles of snsde_scores.hip: a workgroup of four waves takes (o, g, 64 adjacent columns),
// stages the (N, 64) slab in LDS, wave k owns the quarter n in [k N / 4, (k + 1) N / 4) and walks j = 0 .. N-1 for four x_n at a
// time (the quantile kernels: eight); the integer counts of the unweighted kernels become select-and-adds of w_j, j ascending.  The statistics kernels give each
// WAVE its own (g, 64 columns) item and weight rows; a lane walks its column n ascending.
// Determinism: no atomics, nothing depends on the grid or on pointer alignment (scalar loads and stores only).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"
#include "snsde_sample_set.h"      // the column tiles (ST, LANES, WAVES, Dims, Tile, tile_of, row_of, stage, dims_ok), sign0, Norm, normalise

namespace {

constexpr int RB = 4;               // x_n held in registers per walk over the slab
constexpr int MAX_Q = 8;            // quantile levels per call
constexpr int SUM_ROWS = 4 * WAVES; // slab rows the CRPS kernels reuse for the quarter sums
constexpr int META = 64;            // floats after the two weight rows: D', P, F

struct QLevels {
    int32_t n_q;
    float q[MAX_Q];
};

// wave 0 normalises the tile's group into the block's rows and leaves (D', P, F) behind them
__device__ __forceinline__ void normalise_block(const float* __restrict__ logw, const Tile& tl, const Dims& d, float* wrow, int wave, int lane) {
    if (wave == 0) {
        const Norm nm = normalise(logw + tl.og * d.N, d.N, wrow, wrow + MAX_N, lane);
        if (lane == 0) {
            wrow[2 * MAX_N + 0] = nm.Dp;
            wrow[2 * MAX_N + 1] = nm.P;
            wrow[2 * MAX_N + 2] = (float)nm.F;
        }
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
// mean = sum_n fmaf(w_n, x_n, .), var = (sum_n fmaf(w_n, d d, .)) / D', d = x_n - mean: live n ascending
__global__ void __launch_bounds__(ST) snsde_sample_stats_weighted_kernel(const float* __restrict__ ys, const float* __restrict__ logw,
                                                                          int64_t items, int64_t wtiles, int32_t S, int32_t W,
                                                                          float* __restrict__ mean, float* __restrict__ var) {
    __shared__ float rows[WAVES][2 * MAX_N];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    float* wrow = rows[wave];
    const float* lrow = wrow + MAX_N;
    const int64_t quads = (items + WAVES - 1) / WAVES;
    for (int64_t qd = blockIdx.x; qd < quads; qd += gridDim.x) {
        const int64_t item = qd * WAVES + wave;
        const bool valid = item < items;
        const int64_t g = valid ? item / wtiles : 0;
        const int64_t col = (item - g * wtiles) * LANES + lane;
        const bool live = valid && col < W;
        __syncthreads();      // (the rows of the last item have been read)
        Norm nm;
        nm.Dp = 0.0f;
        if (valid) nm = normalise(logw + g * S, S, wrow, wrow + MAX_N, lane);
        __syncthreads();
        if (!live) continue;
        const float* src = ys + (g * S) * (int64_t)W + col;
        float m = 0.0f;
        for (int n = 0; n < S; ++n)
            if (lrow[n] == 0.0f) m = fmaf(wrow[n], src[(int64_t)n * W], m);
        mean[g * W + col] = m;
        if (var) {
            float ss = 0.0f;
            for (int n = 0; n < S; ++n) {
                if (lrow[n] == 0.0f) {
                    const float dv = __fsub_rn(src[(int64_t)n * W], m);
                    ss = fmaf(wrow[n], __fmul_rn(dv, dv), ss);
                }
            }
            var[g * W + col] = __fdiv_rn(ss, nm.Dp);
        }
    }
}

// grad_ys[n] = w_n fmaf(c, x_n - mean, grad_mean), c = (2 grad_var) / D'; without grad_var: w_n grad_mean; a dead sample: 0
__global__ void __launch_bounds__(ST) snsde_sample_stats_weighted_backward_kernel(const float* __restrict__ gmean, const float* __restrict__ gvar,
                                                                                   const float* __restrict__ ys, const float* __restrict__ logw,
                                                                                   const float* __restrict__ mean, int64_t items, int64_t wtiles,
                                                                                   int32_t S, int32_t W, float* __restrict__ gys) {
    __shared__ float rows[WAVES][2 * MAX_N];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    float* wrow = rows[wave];
    const float* lrow = wrow + MAX_N;
    const int64_t quads = (items + WAVES - 1) / WAVES;
    for (int64_t qd = blockIdx.x; qd < quads; qd += gridDim.x) {
        const int64_t item = qd * WAVES + wave;
        const bool valid = item < items;
        const int64_t g = valid ? item / wtiles : 0;
        const int64_t col = (item - g * wtiles) * LANES + lane;
        const bool live = valid && col < W;
        __syncthreads();
        Norm nm;
        nm.Dp = 0.0f;
        if (valid) nm = normalise(logw + g * S, S, wrow, wrow + MAX_N, lane);
        __syncthreads();
        if (!live) continue;
        const int64_t row = (g * S) * (int64_t)W + col;
        const float a = gmean[g * W + col];
        float c = 0.0f, m = 0.0f;
        if (gvar) {
            c = __fdiv_rn(__fmul_rn(2.0f, gvar[g * W + col]), nm.Dp);
            m = mean[g * W + col];
        }
        for (int n = 0; n < S; ++n) {
            float o = 0.0f;
            if (lrow[n] == 0.0f) o = gvar ? __fmul_rn(wrow[n], fmaf(c, __fsub_rn(ys[row + (int64_t)n * W], m), a)) : __fmul_rn(wrow[n], a);
            gys[row + (int64_t)n * W] = o;
        }
    }
}

// ---- CRPS ------------------------------------------------------------------------------------------------------------------
// lt[r] = sum_j w_j [x_j < xn[r]], gt[r] = sum_j w_j [x_j > xn[r]], j ascending (a dead j has w_j = 0 exactly: it adds nothing)
__device__ __forceinline__ void strict_sums(const float* col, const float* wrow, int N, const float (&xn)[RB], float (&lt)[RB], float (&gt)[RB]) {
#pragma unroll
    for (int r = 0; r < RB; ++r) lt[r] = gt[r] = 0.0f;
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
        const float xj = col[j * LANES], wj = wrow[j];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            lt[r] = __fadd_rn(lt[r], xj < xn[r] ? wj : 0.0f);
            gt[r] = __fadd_rn(gt[r], xj > xn[r] ? wj : 0.0f);
        }
    }
}

// crps = sum w_n |d_n| - (sum (w_n C_n) d_n) / D;  rank = sum w_n [x_n < y], ties = sum w_n [x_n == y]
__global__ void __launch_bounds__(ST) snsde_sample_crps_weighted_kernel(const float* __restrict__ ys, const float* __restrict__ target,
                                                                         const float* __restrict__ logw, Dims d, int32_t fair,
                                                                         float* __restrict__ crps, float* __restrict__ rank,
                                                                         float* __restrict__ ties) {
    extern __shared__ float slab[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const int rows = d.N > SUM_ROWS ? d.N : SUM_ROWS;
    float* wrow = slab + rows * LANES;
    const float* lrow = wrow + MAX_N;
    const float* col = slab + lane;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();      // (the last tile's sums and rows have been read)
        stage(ys, tl, d, slab, wave, lane);
        normalise_block(logw, tl, d, wrow, wave, lane);
        const float y = tl.live ? target[tl.out] : 0.0f;
        __syncthreads();
        const float D = fair ? wrow[2 * MAX_N] : 1.0f;
        float A = 0.0f, B = 0.0f, below = 0.0f, equal = 0.0f;
        for (int nb = n0; nb < n1; nb += RB) {
            float xn[RB], lt[RB], gt[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) xn[r] = col[(nb + r < n1 ? nb + r : n1 - 1) * LANES];
            strict_sums(col, wrow, d.N, xn, lt, gt);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (nb + r < n1 && lrow[nb + r] == 0.0f) {
                    const float wn = wrow[nb + r], dn = __fsub_rn(xn[r], y);
                    A = fmaf(wn, fabsf(dn), A);
                    B = fmaf(__fmul_rn(wn, __fsub_rn(lt[r], gt[r])), dn, B);
                    below = fmaf(wn, dn < 0.0f ? 1.0f : 0.0f, below);      // (a product by 0 or 1: exact, and NaN where w_n is)
                    equal = fmaf(wn, dn == 0.0f ? 1.0f : 0.0f, equal);
                }
            }
        }
        __syncthreads();      // every wave is done with the slab: its first rows now carry the quarter sums
        slab[(wave * 4 + 0) * LANES + lane] = A;
        slab[(wave * 4 + 1) * LANES + lane] = B;
        slab[(wave * 4 + 2) * LANES + lane] = below;
        slab[(wave * 4 + 3) * LANES + lane] = equal;
        __syncthreads();
        if (wave == 0 && tl.live) {
            float s[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i] = slab[i * LANES + lane];
#pragma unroll
                for (int k = 1; k < WAVES; ++k) s[i] = __fadd_rn(s[i], slab[(k * 4 + i) * LANES + lane]);
            }
            crps[tl.out] = __fsub_rn(s[0], __fdiv_rn(s[1], D));
            if (rank) rank[tl.out] = s[2];
            if (ties) ties[tl.out] = s[3];
        }
    }
}

// grad_ys[n] = g (w_n (sign(d_n) - C_n / D));  grad_target = -(g sum_n fmaf(w_n, sign(d_n), .)); a dead sample: 0
__global__ void __launch_bounds__(ST) snsde_sample_crps_weighted_backward_kernel(const float* __restrict__ gcrps, const float* __restrict__ ys,
                                                                                  const float* __restrict__ target, const float* __restrict__ logw,
                                                                                  Dims d, int32_t fair, float* __restrict__ gys,
                                                                                  float* __restrict__ gtarget) {
    extern __shared__ float slab[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const int rows = d.N > SUM_ROWS ? d.N : SUM_ROWS;
    float* wrow = slab + rows * LANES;
    const float* lrow = wrow + MAX_N;
    const float* col = slab + lane;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();
        stage(ys, tl, d, slab, wave, lane);
        normalise_block(logw, tl, d, wrow, wave, lane);
        const float y = tl.live ? target[tl.out] : 0.0f, g = tl.live ? gcrps[tl.out] : 0.0f;
        __syncthreads();
        const float D = fair ? wrow[2 * MAX_N] : 1.0f;
        float signs = 0.0f;
        for (int nb = n0; nb < n1; nb += RB) {
            float xn[RB], lt[RB], gt[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) xn[r] = col[(nb + r < n1 ? nb + r : n1 - 1) * LANES];
            strict_sums(col, wrow, d.N, xn, lt, gt);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (nb + r < n1) {
                    float o = 0.0f;
                    if (lrow[nb + r] == 0.0f) {
                        const float wn = wrow[nb + r], sg = sign0(__fsub_rn(xn[r], y));
                        signs = fmaf(wn, sg, signs);
                        o = __fmul_rn(g, __fmul_rn(wn, __fsub_rn(sg, __fdiv_rn(__fsub_rn(lt[r], gt[r]), D))));
                    }
                    if (tl.live) gys[tl.base + row_of(nb + r, d)] = o;
                }
            }
        }
        if (gtarget) {      // (uniform over the block)
            __syncthreads();
            slab[wave * LANES + lane] = signs;
            __syncthreads();
            if (wave == 0 && tl.live) {
                float s = slab[lane];
#pragma unroll
                for (int k = 1; k < WAVES; ++k) s = __fadd_rn(s, slab[k * LANES + lane]);
                gtarget[tl.out] = -__fmul_rn(g, s);
            }
        }
    }
}

// ---- quantiles -------------------------------------------------------------------------------------------------------------
// LDS of the quantile kernels, in floats: the slab (N, 64) | nodes p (max(N, 32), 64) | w (256) | live (256) | D', P, F (64) | NaN
// flags (4, 64) | then N x 64 bytes: perm[r][lane] = the sample that holds rank r.  The backward's brackets (MAX_Q, 4, 64) take the
// place of the nodes once every wave has searched them.
constexpr int RQ = 8;               // x_n held in registers per walk of the quantile kernels (LDS, not registers, bounds their occupancy)
constexpr int BRK_ROWS = MAX_Q * 4; // rows of the brackets

// ranks among the live samples, ties by index, and the cumulative weight in front of each: rk[r] = #{live j ranked before n[r]},
// A[r] = sum of their w_j, j ascending.  A dead j reads as NaN (x_j + lrow[j]) - compared with nobody; a NaN sample has no rank (-1).
__device__ __forceinline__ void ranks_and_mass(const float* col, const float* wrow, const float* lrow, int N, const float (&xn)[RQ],
                                               const int (&n)[RQ], int (&rk)[RQ], float (&A)[RQ]) {
#pragma unroll
    for (int r = 0; r < RQ; ++r) { rk[r] = 0; A[r] = 0.0f; }
#pragma unroll 2
    for (int j = 0; j < N; ++j) {
        const float xj = __fadd_rn(col[j * LANES], lrow[j]), wj = wrow[j];
#pragma unroll
        for (int r = 0; r < RQ; ++r) {
            const bool before = (xj < xn[r]) | ((xj == xn[r]) & (j < n[r]));      // (no short circuit: no branch)
            rk[r] += before ? 1 : 0;
            A[r] = __fadd_rn(A[r], before ? wj : 0.0f);
        }
    }
#pragma unroll
    for (int r = 0; r < RQ; ++r) rk[r] = xn[r] != xn[r] ? -1 : rk[r];
}

struct QLds {
    float *slab, *pnode, *wrow, *lrow, *nanf, *brk;
    uint8_t* perm;
};

__device__ __forceinline__ QLds qlds_of(float* base, int N) {
    QLds q;
    q.slab = base;
    q.pnode = q.slab + N * LANES;
    q.wrow = q.pnode + (N > BRK_ROWS ? N : BRK_ROWS) * LANES;
    q.lrow = q.wrow + MAX_N;
    q.nanf = q.lrow + MAX_N + META;
    q.brk = q.pnode;
    q.perm = reinterpret_cast<uint8_t*>(q.nanf + WAVES * LANES);
    return q;
}

// the walk of a wave over its quarter: the node p_n of every live, ranked sample to pnode[n], its index to perm[rank]; returns
// whether the quarter holds a live NaN
__device__ __forceinline__ float rank_quarter(const QLds& L, const Dims& d, int F, int n0, int n1, int lane) {
    const float* col = L.slab + lane;
    float has_nan = 0.0f;
    for (int nb = n0; nb < n1; nb += RQ) {
        float xn[RQ], A[RQ];
        int n[RQ], rk[RQ];
#pragma unroll
        for (int r = 0; r < RQ; ++r) {
            n[r] = nb + r < n1 ? nb + r : n1 - 1;
            xn[r] = col[n[r] * LANES];
        }
        ranks_and_mass(col, L.wrow, L.lrow, d.N, xn, n, rk, A);
#pragma unroll
        for (int r = 0; r < RQ; ++r) {
            if (nb + r < n1 && L.lrow[n[r]] == 0.0f) {
                if (rk[r] < 0) has_nan = 1.0f;
                else {
                    const float p = rk[r] == 0 ? 0.0f : rk[r] == F - 1 ? 1.0f : __fdiv_rn(A[r], __fsub_rn(1.0f, L.wrow[n[r]]));
                    L.pnode[n[r] * LANES + lane] = p;
                    L.perm[rk[r] * LANES + lane] = (uint8_t)n[r];
                }
            }
        }
    }
    return has_nan;
}

struct Bracket {
    int lo, hi;        // sample indices; hi = -1: the value is x_lo
    float frac;
};

// lo = the sample of largest rank with p <= q (rank 0 has p = 0 <= q), hi the sample of the next rank
__device__ __forceinline__ Bracket bracket_of(const QLds& L, int F, float q, int lane) {
    int r = F - 1;
    for (; r > 0; --r)
        if (L.pnode[L.perm[r * LANES + lane] * LANES + lane] <= q) break;
    Bracket b;
    b.lo = L.perm[r * LANES + lane];
    b.hi = -1;
    b.frac = 0.0f;
    if (r < F - 1) {
        const int h = L.perm[(r + 1) * LANES + lane];
        const float plo = L.pnode[b.lo * LANES + lane], phi = L.pnode[h * LANES + lane];
        b.frac = fminf(fmaxf(__fdiv_rn(__fsub_rn(q, plo), __fsub_rn(phi, plo)), 0.0f), 1.0f);
        if (b.frac != 0.0f) b.hi = h;
    }
    return b;
}

__global__ void __launch_bounds__(ST) snsde_sample_quantiles_weighted_kernel(const float* __restrict__ ys, const float* __restrict__ logw, Dims d,
                                                                              QLevels ql, float* __restrict__ outq) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const QLds L = qlds_of(lds, d.N);
    const int64_t plane = d.outer * d.G * d.W;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();
        stage(ys, tl, d, L.slab, wave, lane);
        normalise_block(logw, tl, d, L.wrow, wave, lane);
        __syncthreads();
        const float P = L.wrow[2 * MAX_N + 1];
        const int F = (int)L.wrow[2 * MAX_N + 2];
        L.nanf[wave * LANES + lane] = rank_quarter(L, d, F, n0, n1, lane);
        __syncthreads();
        bool bad = P != P;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) bad |= L.nanf[k * LANES + lane] != 0.0f;
        for (int q = wave; q < ql.n_q; q += WAVES) {      // wave k answers the levels k, k + 4
            float v = __builtin_nanf("");
            if (!bad) {
                const Bracket b = bracket_of(L, F, ql.q[q], lane);
                const float a = L.slab[b.lo * LANES + lane];
                v = b.hi < 0 ? a : fmaf(b.frac, __fsub_rn(L.slab[b.hi * LANES + lane], a), a);
            }
            if (tl.live) outq[q * plane + tl.out] = v;
        }
    }
}

// grad_ys[lo_q] += g_q (1 - frac_q), grad_ys[hi_q] += g_q frac_q, q ascending; zeros elsewhere; a column with a live NaN: zeros; an
// unusable weight set: NaN
__global__ void __launch_bounds__(ST) snsde_sample_quantiles_weighted_backward_kernel(const float* __restrict__ gout, const float* __restrict__ ys,
                                                                                       const float* __restrict__ logw, Dims d, QLevels ql,
                                                                                       float* __restrict__ gys) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const QLds L = qlds_of(lds, d.N);
    const int64_t plane = d.outer * d.G * d.W;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();
        stage(ys, tl, d, L.slab, wave, lane);
        normalise_block(logw, tl, d, L.wrow, wave, lane);
        __syncthreads();
        const float P = L.wrow[2 * MAX_N + 1];
        const int F = (int)L.wrow[2 * MAX_N + 2];
        L.nanf[wave * LANES + lane] = rank_quarter(L, d, F, n0, n1, lane);
        __syncthreads();
        bool has_nan = false;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) has_nan |= L.nanf[k * LANES + lane] != 0.0f;
        const bool badw = P != P;
        float lo[2], hi[2], glo[2], ghi[2];      // wave k answers the levels k and k + 4
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = wave + i * WAVES;
            lo[i] = hi[i] = -1.0f;
            glo[i] = ghi[i] = 0.0f;
            if (q < ql.n_q && !badw && !has_nan) {
                const Bracket b = bracket_of(L, F, ql.q[q], lane);
                const float g = tl.live ? gout[q * plane + tl.out] : 0.0f;
                lo[i] = (float)b.lo;
                hi[i] = (float)b.hi;
                glo[i] = __fmul_rn(g, __fsub_rn(1.0f, b.frac));
                ghi[i] = __fmul_rn(g, b.frac);
            }
        }
        __syncthreads();      // every wave has searched the nodes: their place now carries the brackets
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = wave + i * WAVES;
            if (q < ql.n_q) {
                L.brk[(q * 4 + 0) * LANES + lane] = lo[i];
                L.brk[(q * 4 + 1) * LANES + lane] = hi[i];
                L.brk[(q * 4 + 2) * LANES + lane] = glo[i];
                L.brk[(q * 4 + 3) * LANES + lane] = ghi[i];
            }
        }
        __syncthreads();
        int nlo[MAX_Q], nhi[MAX_Q];
        float wlo[MAX_Q], whi[MAX_Q];
#pragma unroll
        for (int q = 0; q < MAX_Q; ++q) {
            const bool on = q < ql.n_q;
            nlo[q] = on ? (int)L.brk[(q * 4 + 0) * LANES + lane] : -1;
            nhi[q] = on ? (int)L.brk[(q * 4 + 1) * LANES + lane] : -1;
            wlo[q] = on ? L.brk[(q * 4 + 2) * LANES + lane] : 0.0f;
            whi[q] = on ? L.brk[(q * 4 + 3) * LANES + lane] : 0.0f;
        }
        for (int n = n0; n < n1; ++n) {
            float acc = 0.0f;
            if (badw) acc = __builtin_nanf("");
            else if (L.lrow[n] == 0.0f) {
#pragma unroll
                for (int q = 0; q < MAX_Q; ++q) {
                    if (nlo[q] == n) acc = __fadd_rn(acc, wlo[q]);
                    if (nhi[q] == n) acc = __fadd_rn(acc, whi[q]);
                }
            }
            if (tl.live) gys[tl.base + row_of(n, d)] = acc;
        }
    }
}

bool levels_ok(int32_t n_q, const float* q, QLevels* ql) {
    if (n_q < 1 || n_q > MAX_Q) return false;
    ql->n_q = n_q;
    for (int i = 0; i < MAX_Q; ++i) ql->q[i] = 0.0f;
    for (int i = 0; i < n_q; ++i) {
        if (!(q[i] >= 0.0f && q[i] <= 1.0f)) return false;
        ql->q[i] = q[i];
    }
    return true;
}

unsigned grid_of(int64_t tiles) { return (unsigned)(tiles < 8192 ? tiles : 8192); }      // (the kernels stride over the rest)
size_t crps_lds(const Dims& d) { return ((size_t)(d.N > SUM_ROWS ? d.N : SUM_ROWS) * LANES + 2 * MAX_N + META) * sizeof(float); }
size_t quant_lds(const Dims& d) {
    return ((size_t)(d.N + (d.N > BRK_ROWS ? d.N : BRK_ROWS)) * LANES + 2 * MAX_N + META + WAVES * LANES) * sizeof(float) + (size_t)d.N * LANES;
}

SnsdeLdsAttr crps_attr, crps_bwd_attr, quant_attr, quant_bwd_attr;

}  // namespace

extern "C" int snsde_sample_stats_weighted(const float* ys, const float* logw, int64_t groups, int32_t samples, int32_t width, float* mean,
                                           float* var, void* hip_stream) {
    if (!ys || !logw || !mean) return SNSDE_ERR_NULL;
    if (groups <= 0 || samples <= 0 || width <= 0 || samples > MAX_N) return SNSDE_ERR_DIMS;
    if (var && samples < 2) return SNSDE_ERR_DIMS;
    if (groups > INT64_MAX / samples / width) return SNSDE_ERR_DIMS;
    const int64_t wtiles = ((int64_t)width + LANES - 1) / LANES, items = groups * wtiles;
    hipLaunchKernelGGL(snsde_sample_stats_weighted_kernel, dim3(grid_of((items + WAVES - 1) / WAVES)), dim3(ST), 0,
                       static_cast<hipStream_t>(hip_stream), ys, logw, items, wtiles, samples, width, mean, var);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_stats_weighted_backward(const float* grad_mean, const float* grad_var, const float* ys, const float* logw,
                                                    const float* mean, int64_t groups, int32_t samples, int32_t width, float* grad_ys,
                                                    void* hip_stream) {
    if (!grad_mean || !logw || !grad_ys || (grad_var && (!ys || !mean))) return SNSDE_ERR_NULL;
    if (groups <= 0 || samples <= 0 || width <= 0 || samples > MAX_N) return SNSDE_ERR_DIMS;
    if (grad_var && samples < 2) return SNSDE_ERR_DIMS;
    if (groups > INT64_MAX / samples / width) return SNSDE_ERR_DIMS;
    const int64_t wtiles = ((int64_t)width + LANES - 1) / LANES, items = groups * wtiles;
    hipLaunchKernelGGL(snsde_sample_stats_weighted_backward_kernel, dim3(grid_of((items + WAVES - 1) / WAVES)), dim3(ST), 0,
                       static_cast<hipStream_t>(hip_stream), grad_mean, grad_var, ys, logw, mean, items, wtiles, samples, width, grad_ys);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_crps_weighted(const float* ys, const float* target, const float* logw, int64_t outer, int32_t members,
                                          int64_t groups, int32_t samples, int32_t width, int32_t fair, float* crps, float* rank, float* ties,
                                          void* hip_stream) {
    if (!ys || !target || !logw || !crps) return SNSDE_ERR_NULL;
    Dims d;
    if (!dims_ok(outer, members, groups, samples, width, &d)) return SNSDE_ERR_DIMS;
    if (fair && d.N < 2) return SNSDE_ERR_DIMS;
    const size_t lds = crps_lds(d);
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(snsde_sample_crps_weighted_kernel), lds, crps_attr);
    if (rc != SNSDE_OK) return rc;
    hipLaunchKernelGGL(snsde_sample_crps_weighted_kernel, dim3(grid_of(d.tiles)), dim3(ST), lds, static_cast<hipStream_t>(hip_stream), ys, target,
                       logw, d, fair != 0, crps, rank, ties);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_crps_weighted_backward(const float* grad_crps, const float* ys, const float* target, const float* logw,
                                                   int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                                   int32_t fair, float* grad_ys, float* grad_target, void* hip_stream) {
    if (!grad_crps || !ys || !target || !logw || !grad_ys) return SNSDE_ERR_NULL;
    Dims d;
    if (!dims_ok(outer, members, groups, samples, width, &d)) return SNSDE_ERR_DIMS;
    if (fair && d.N < 2) return SNSDE_ERR_DIMS;
    const size_t lds = crps_lds(d);
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(snsde_sample_crps_weighted_backward_kernel), lds, crps_bwd_attr);
    if (rc != SNSDE_OK) return rc;
    hipLaunchKernelGGL(snsde_sample_crps_weighted_backward_kernel, dim3(grid_of(d.tiles)), dim3(ST), lds, static_cast<hipStream_t>(hip_stream),
                       grad_crps, ys, target, logw, d, fair != 0, grad_ys, grad_target);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_quantiles_weighted(const float* ys, const float* logw, int64_t outer, int32_t members, int64_t groups,
                                               int32_t samples, int32_t width, int32_t n_q, const float* q, float* out, void* hip_stream) {
    if (!ys || !logw || !q || !out) return SNSDE_ERR_NULL;
    Dims d;
    QLevels ql;
    if (!dims_ok(outer, members, groups, samples, width, &d) || !levels_ok(n_q, q, &ql)) return SNSDE_ERR_DIMS;
    if (d.tiles > INT64_MAX / LANES / n_q) return SNSDE_ERR_DIMS;      // (the (n_q, outer, groups, width) output)
    const size_t lds = quant_lds(d);
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(snsde_sample_quantiles_weighted_kernel), lds, quant_attr);
    if (rc != SNSDE_OK) return rc;
    hipLaunchKernelGGL(snsde_sample_quantiles_weighted_kernel, dim3(grid_of(d.tiles)), dim3(ST), lds, static_cast<hipStream_t>(hip_stream), ys,
                       logw, d, ql, out);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_quantiles_weighted_backward(const float* grad_out, const float* ys, const float* logw, int64_t outer,
                                                        int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t n_q,
                                                        const float* q, float* grad_ys, void* hip_stream) {
    if (!grad_out || !ys || !logw || !q || !grad_ys) return SNSDE_ERR_NULL;
    Dims d;
    QLevels ql;
    if (!dims_ok(outer, members, groups, samples, width, &d) || !levels_ok(n_q, q, &ql)) return SNSDE_ERR_DIMS;
    if (d.tiles > INT64_MAX / LANES / n_q) return SNSDE_ERR_DIMS;
    const size_t lds = quant_lds(d);
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(snsde_sample_quantiles_weighted_backward_kernel), lds, quant_bwd_attr);
    if (rc != SNSDE_OK) return rc;
    hipLaunchKernelGGL(snsde_sample_quantiles_weighted_backward_kernel, dim3(grid_of(d.tiles)), dim3(ST), lds,
                       static_cast<hipStream_t>(hip_stream), grad_out, ys, logw, d, ql, grad_ys);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
