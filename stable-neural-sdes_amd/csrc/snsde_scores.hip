// Scores of sample paths against an observation, and their adjoints (include/snsde.h: snsde_sample_crps, snsde_sample_crps_backward,
// snsde_sample_quantiles, snsde_sample_quantiles_backward).
// ys is (outer, M, G, S, W); the pooled sample set of an output element (o, g, w) is x_n, n = m S + s, N = M S of them.  The members
// axis is addressing only (member_stride = G S W), so a pooled call and the members = 1 call on the permuted (outer G, M S, W)
// tensor run the same arithmetic.
// Ownership as in snsde_stats.hip: adjacent lanes own adjacent columns of one group.  A workgroup of four waves takes one tile
// (o, g, 64 adjacent columns), stages its (N, 64) slab once in LDS - row-major, lane j reads bank j of every row: conflict-free
// ds_read_b32 - and each lane walks its own column of the slab.  The N^2 comparisons per element are the whole cost; they are
// split over the waves by n: wave k owns the contiguous quarter n in [k N / 4, (k + 1) N / 4), holds four x_n in registers and
// compares them against every x_j it reads (one LDS read per four pairs).
// Determinism: no atomics, nothing depends on the grid.  The two sums of the score run n ascending inside a quarter, and the four
// quarter sums are added k ascending; every count is an integer.  The same bits on every launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_sample_set.h"      // the column tiles (ST, LANES, WAVES, Dims, Tile, tile_of, row_of, stage, dims_ok), MAX_N (x 256 B = 64 KB of LDS), sign0

namespace {

constexpr int RB = 4;               // x_n held in registers per walk over the slab
constexpr int MAX_Q = 8;            // quantiles per call (their k / frac travel in the kernel's argument struct)
constexpr int XROWS = MAX_Q * 2;    // rows of the exchange area (MAX_Q * 2 * 64 floats), which aliases the slab
constexpr int MIN_ROWS = XROWS + WAVES;   // slab rows allocated at least: the exchange area and one row of NaN flags per wave

struct QArgs {
    int32_t n_q;
    int32_t k[MAX_Q];
    float frac[MAX_Q];
};

// strict counts of RB samples against the whole column: lt[r] = #{j : x_j < xn[r]}, gt[r] = #{j : x_j > xn[r]}
__device__ __forceinline__ void strict_counts(const float* col, int N, const float (&xn)[RB], int (&lt)[RB], int (&gt)[RB]) {
#pragma unroll
    for (int r = 0; r < RB; ++r) lt[r] = gt[r] = 0;
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
        const float xj = col[j * LANES];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            lt[r] += xj < xn[r] ? 1 : 0;
            gt[r] += xj > xn[r] ? 1 : 0;
        }
    }
}

// permutation ranks, ties broken by index: rk[r] = #{j : x_j < xn[r]} + #{j < n[r] : x_j == xn[r]}; a NaN has no rank: -1, which
// no level asks for (both comparisons are false for it and nothing counts it: the finite samples rank among themselves)
__device__ __forceinline__ void perm_ranks(const float* col, int N, const float (&xn)[RB], const int (&n)[RB], int (&rk)[RB]) {
#pragma unroll
    for (int r = 0; r < RB; ++r) rk[r] = 0;
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
        const float xj = col[j * LANES];
#pragma unroll
        for (int r = 0; r < RB; ++r) rk[r] += (xj < xn[r] || (xj == xn[r] && j < n[r])) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) rk[r] = xn[r] != xn[r] ? -1 : rk[r];
}

// crps = (sum |d_n|) / N - (sum c_n d_n) / (N D);  rank = #{x_n < y}, ties = #{x_n == y}
__global__ void __launch_bounds__(ST) snsde_sample_crps_kernel(const float* __restrict__ ys, const float* __restrict__ target, Dims d, int32_t D,
                                                               float* __restrict__ crps, float* __restrict__ rank, float* __restrict__ ties) {
    extern __shared__ float slab[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const float fN = (float)d.N, fND = (float)(d.N * D);      // (N D <= 65536: exact)
    const float* col = slab + lane;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();      // (the last tile's exchange area has been read)
        stage(ys, tl, d, slab, wave, lane);
        const float y = tl.live ? target[tl.out] : 0.0f;
        __syncthreads();
        float A = 0.0f, B = 0.0f, below = 0.0f, equal = 0.0f;
        for (int nb = n0; nb < n1; nb += RB) {
            float xn[RB];
            int lt[RB], gt[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) xn[r] = col[(nb + r < n1 ? nb + r : n1 - 1) * LANES];
            strict_counts(col, d.N, xn, lt, gt);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (nb + r < n1) {
                    const float dn = xn[r] - y;
                    A += fabsf(dn);
                    B = fmaf((float)(lt[r] - gt[r]), dn, B);
                    below += dn < 0.0f ? 1.0f : 0.0f;
                    equal += dn == 0.0f ? 1.0f : 0.0f;
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
                for (int k = 1; k < WAVES; ++k) s[i] += slab[(k * 4 + i) * LANES + lane];
            }
            crps[tl.out] = s[0] / fN - s[1] / fND;
            if (rank) rank[tl.out] = s[2];
            if (ties) ties[tl.out] = s[3];
        }
    }
}

// grad_ys[n] = g (sign(d_n) / N - c_n / (N D));  grad_target = -(g sum_n sign(d_n)) / N
__global__ void __launch_bounds__(ST) snsde_sample_crps_backward_kernel(const float* __restrict__ gcrps, const float* __restrict__ ys,
                                                                        const float* __restrict__ target, Dims d, int32_t D,
                                                                        float* __restrict__ gys, float* __restrict__ gtarget) {
    extern __shared__ float slab[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const float fN = (float)d.N, fND = (float)(d.N * D);
    const float* col = slab + lane;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();
        stage(ys, tl, d, slab, wave, lane);
        const float y = tl.live ? target[tl.out] : 0.0f, g = tl.live ? gcrps[tl.out] : 0.0f;
        __syncthreads();
        float signs = 0.0f;      // (an integer: exact in any order)
        for (int nb = n0; nb < n1; nb += RB) {
            float xn[RB];
            int lt[RB], gt[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) xn[r] = col[(nb + r < n1 ? nb + r : n1 - 1) * LANES];
            strict_counts(col, d.N, xn, lt, gt);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (nb + r < n1) {
                    const float sg = sign0(xn[r] - y);
                    signs += sg;
                    if (tl.live) gys[tl.base + row_of(nb + r, d)] = g * (sg / fN - (float)(lt[r] - gt[r]) / fND);
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
                for (int k = 1; k < WAVES; ++k) s += slab[k * LANES + lane];
                gtarget[tl.out] = -(g * s) / fN;
            }
        }
    }
}

// out[q] = x_(k_q), or fmaf(frac_q, x_(k_q + 1) - x_(k_q), x_(k_q)) where frac_q != 0; NaN at every level where the column holds a
// NaN.  Such a column has fewer ranked samples than levels may ask for, so some exchange rows are never written: every wave flags
// the NaNs of its own quarter, and the epilogue reads no exchange row of a flagged column.
__global__ void __launch_bounds__(ST) snsde_sample_quantiles_kernel(const float* __restrict__ ys, Dims d, QArgs qa, float* __restrict__ outq) {
    extern __shared__ float slab[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const float* col = slab + lane;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();
        stage(ys, tl, d, slab, wave, lane);
        __syncthreads();
        float lo[MAX_Q], hi[MAX_Q];
        unsigned found_lo = 0, found_hi = 0;      // (a rank is held by at most one sample: one wave finds each order statistic)
        float has_nan = 0.0f;
#pragma unroll
        for (int q = 0; q < MAX_Q; ++q) lo[q] = hi[q] = 0.0f;
        for (int nb = n0; nb < n1; nb += RB) {
            float xn[RB];
            int n[RB], rk[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                n[r] = nb + r < n1 ? nb + r : n1 - 1;
                xn[r] = col[n[r] * LANES];
            }
            perm_ranks(col, d.N, xn, n, rk);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (nb + r < n1) {
                    has_nan = rk[r] < 0 ? 1.0f : has_nan;
#pragma unroll
                    for (int q = 0; q < MAX_Q; ++q) {
                        if (q < qa.n_q && rk[r] == qa.k[q]) { lo[q] = xn[r]; found_lo |= 1u << q; }
                        if (q < qa.n_q && rk[r] == qa.k[q] + 1) { hi[q] = xn[r]; found_hi |= 1u << q; }
                    }
                }
            }
        }
        __syncthreads();      // every wave is done with the slab: its first rows now carry the order statistics
#pragma unroll
        for (int q = 0; q < MAX_Q; ++q) {
            if (found_lo & (1u << q)) slab[(q * 2 + 0) * LANES + lane] = lo[q];
            if (found_hi & (1u << q)) slab[(q * 2 + 1) * LANES + lane] = hi[q];
        }
        slab[(XROWS + wave) * LANES + lane] = has_nan;
        __syncthreads();
        if (wave == 0 && tl.live) {
            const int64_t plane = d.outer * d.G * d.W;
            bool bad = false;
#pragma unroll
            for (int k = 0; k < WAVES; ++k) bad |= slab[(XROWS + k) * LANES + lane] != 0.0f;
#pragma unroll
            for (int q = 0; q < MAX_Q; ++q) {
                if (q < qa.n_q) {
                    float v = __builtin_nanf("");
                    if (!bad) {
                        const float a = slab[(q * 2 + 0) * LANES + lane];
                        v = a;
                        if (qa.frac[q] != 0.0f) v = fmaf(qa.frac[q], slab[(q * 2 + 1) * LANES + lane] - a, a);
                    }
                    outq[q * plane + tl.out] = v;
                }
            }
        }
    }
}

// grad_ys[n] = sum_q g_q (1 - frac_q) [rank_n == k_q] + g_q frac_q [rank_n == k_q + 1], q ascending; exact zeros elsewhere.  In a
// column that holds a NaN (forward: NaN) a NaN sample has no rank and gets an exact zero; the finite samples get the terms of the
// ranks they hold among themselves, and the terms of ranks nobody holds go nowhere: still a function of the inputs alone.
__global__ void __launch_bounds__(ST) snsde_sample_quantiles_backward_kernel(const float* __restrict__ gout, const float* __restrict__ ys, Dims d,
                                                                             QArgs qa, float* __restrict__ gys) {
    extern __shared__ float slab[];
    const int lane = threadIdx.x & (LANES - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    const int n0 = wave * d.N / WAVES, n1 = (wave + 1) * d.N / WAVES;
    const float* col = slab + lane;
    const int64_t plane = d.outer * d.G * d.W;
    for (int64_t t = blockIdx.x; t < d.tiles; t += gridDim.x) {
        const Tile tl = tile_of(t, d, lane);
        __syncthreads();
        stage(ys, tl, d, slab, wave, lane);
        float glo[MAX_Q], ghi[MAX_Q];
#pragma unroll
        for (int q = 0; q < MAX_Q; ++q) {
            const float g = (q < qa.n_q && tl.live) ? gout[q * plane + tl.out] : 0.0f;
            const float f = q < qa.n_q ? qa.frac[q] : 0.0f;
            glo[q] = g * (1.0f - f);
            ghi[q] = g * f;
        }
        __syncthreads();
        for (int nb = n0; nb < n1; nb += RB) {
            float xn[RB];
            int n[RB], rk[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                n[r] = nb + r < n1 ? nb + r : n1 - 1;
                xn[r] = col[n[r] * LANES];
            }
            perm_ranks(col, d.N, xn, n, rk);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (nb + r < n1 && tl.live) {
                    float acc = 0.0f;
#pragma unroll
                    for (int q = 0; q < MAX_Q; ++q) {
                        if (q < qa.n_q && rk[r] == qa.k[q]) acc += glo[q];
                        if (q < qa.n_q && qa.frac[q] != 0.0f && rk[r] == qa.k[q] + 1) acc += ghi[q];
                    }
                    gys[tl.base + row_of(nb + r, d)] = acc;
                }
            }
        }
    }
}

bool quantiles_ok(int32_t N, int32_t n_q, const int32_t* k, const float* frac, QArgs* qa) {
    if (n_q < 1 || n_q > MAX_Q) return false;
    qa->n_q = n_q;
    for (int q = 0; q < MAX_Q; ++q) { qa->k[q] = 0; qa->frac[q] = 0.0f; }
    for (int q = 0; q < n_q; ++q) {
        if (k[q] < 0 || k[q] > N - 1) return false;
        if (!(frac[q] >= 0.0f && frac[q] < 1.0f)) return false;
        if (k[q] == N - 1 && frac[q] != 0.0f) return false;
        qa->k[q] = k[q];
        qa->frac[q] = frac[q];
    }
    return true;
}

unsigned grid_of(const Dims& d) { return (unsigned)(d.tiles < 8192 ? d.tiles : 8192); }      // (the kernels stride over the rest)
size_t lds_of(const Dims& d) { return (size_t)(d.N > MIN_ROWS ? d.N : MIN_ROWS) * LANES * sizeof(float); }

}  // namespace

extern "C" int snsde_sample_crps(const float* ys, const float* target, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                 int32_t width, int32_t fair, float* crps, float* rank, float* ties, void* hip_stream) {
    if (!ys || !target || !crps) return SNSDE_ERR_NULL;
    Dims d;
    if (!dims_ok(outer, members, groups, samples, width, &d)) return SNSDE_ERR_DIMS;
    if (fair && d.N < 2) return SNSDE_ERR_DIMS;      // (the unbiased estimator divides by N - 1)
    hipLaunchKernelGGL(snsde_sample_crps_kernel, dim3(grid_of(d)), dim3(ST), lds_of(d), static_cast<hipStream_t>(hip_stream), ys, target, d,
                       fair ? d.N - 1 : d.N, crps, rank, ties);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_crps_backward(const float* grad_crps, const float* ys, const float* target, int64_t outer, int32_t members,
                                          int64_t groups, int32_t samples, int32_t width, int32_t fair, float* grad_ys, float* grad_target,
                                          void* hip_stream) {
    if (!grad_crps || !ys || !target || !grad_ys) return SNSDE_ERR_NULL;
    Dims d;
    if (!dims_ok(outer, members, groups, samples, width, &d)) return SNSDE_ERR_DIMS;
    if (fair && d.N < 2) return SNSDE_ERR_DIMS;
    hipLaunchKernelGGL(snsde_sample_crps_backward_kernel, dim3(grid_of(d)), dim3(ST), lds_of(d), static_cast<hipStream_t>(hip_stream), grad_crps,
                       ys, target, d, fair ? d.N - 1 : d.N, grad_ys, grad_target);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_quantiles(const float* ys, int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                      int32_t n_q, const int32_t* k, const float* frac, float* out, void* hip_stream) {
    if (!ys || !k || !frac || !out) return SNSDE_ERR_NULL;
    Dims d;
    QArgs qa;
    if (!dims_ok(outer, members, groups, samples, width, &d) || !quantiles_ok(d.N, n_q, k, frac, &qa)) return SNSDE_ERR_DIMS;
    if (d.tiles > INT64_MAX / LANES / n_q) return SNSDE_ERR_DIMS;      // (the (n_q, outer, groups, width) output)
    hipLaunchKernelGGL(snsde_sample_quantiles_kernel, dim3(grid_of(d)), dim3(ST), lds_of(d), static_cast<hipStream_t>(hip_stream), ys, d, qa, out);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_quantiles_backward(const float* grad_out, const float* ys, int64_t outer, int32_t members, int64_t groups,
                                               int32_t samples, int32_t width, int32_t n_q, const int32_t* k, const float* frac,
                                               float* grad_ys, void* hip_stream) {
    if (!grad_out || !ys || !k || !frac || !grad_ys) return SNSDE_ERR_NULL;
    Dims d;
    QArgs qa;
    if (!dims_ok(outer, members, groups, samples, width, &d) || !quantiles_ok(d.N, n_q, k, frac, &qa)) return SNSDE_ERR_DIMS;
    if (d.tiles > INT64_MAX / LANES / n_q) return SNSDE_ERR_DIMS;
    hipLaunchKernelGGL(snsde_sample_quantiles_backward_kernel, dim3(grid_of(d)), dim3(ST), lds_of(d), static_cast<hipStream_t>(hip_stream),
                       grad_out, ys, d, qa, grad_ys);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
