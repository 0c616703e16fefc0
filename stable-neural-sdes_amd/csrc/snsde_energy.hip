// Energy score of sample paths against an observation, of weighted and of partially observed sample sets, and its adjoint with
// the weights fixed (include/snsde.h: snsde_sample_energy, snsde_sample_energy_backward, snsde_sample_energy_weighted,
// snsde_sample_energy_weighted_backward).  One kernel template; weights (WGT) and mask (MSK) are compile-time variants, and the
// variant with neither is the kernel of the two unweighted entry points.
// ys is (outer, M, G, S, W) as in snsde_sample_set.h; the pooled sample set of a group g is N vectors of V components: V = W, one
// score per (o, g) (path = 0), or V = outer W, component v = o W + w, one score per g (path != 0).  The members and outer axes
// are addressing only.
// Ownership: one workgroup per score.  The N samples and the observation (row N) are the N + 1 rows of one table; rows are taken
// in blocks of four (R = ceil((N + 1) / 4) blocks, the rows past N staged as zeros and masked), and the R (R + 1) / 2 block pairs
// (bi <= bj) - 4 x 4 micro-tiles of row pairs - are dealt to the lanes, tile t = bj (bj + 1) / 2 + bi to lane t mod THREADS.  A
// lane keeps the 16 squared distances of each of its tiles in registers over the whole vector: the columns are consumed in
// chunks of 16, each staged column-major in LDS (slab[c][row], row stride RP = 4 mod 32 words), so a tile reads its two row
// blocks of a column as two 16-byte LDS reads for 16 pairs.  Lanes past V stage zeros and store nothing.  The loads of the next
// chunk are issued into registers before the current one is consumed.
// Buckets by T = R (R + 1) / 2: one wave and one tile per lane (T <= 64: N <= 39), four waves and 1 / 3 / 9 tiles per lane
// (N <= 87 / 151 / 256).
// Mask (MSK).  A column v of a score is observed where mask[v] != 0, or, without a mask tensor and with nan_missing, where the
// target is not NaN; the thread that stages a column decides it (one more load per column and chunk) and stages ZEROS for every
// row of an unobserved column: d = 0 - 0 and fmaf(0, 0, acc) leave every chain as it was, bit for bit, so a masked score has the
// bits of the unmasked kernel on the observed columns alone.  Nothing of ys or target is read there.
// Weights (WGT).  Wave 0 normalises the score's N log-weights on chip while the loads of the first chunk fly (normalise(),
// snsde_sample_set.h): w_n and a live mark (0 live, NaN dead) go to two LDS rows of 272 floats, row N - the observation - as w = 1
// and live, the padding rows as dead, and D', P behind them.  A dead sample is selected out of every pair by its mark, never
// multiplied; in a group whose P is NaN every w_n is NaN, nothing is selected out, and NaN reaches every value by the arithmetic.
// Summation order (a function of N, V, fair and nothing else):
//   squared distance of a pair: one fmaf(d, d, .) chain over v ascending, d = x_iv - x_jv (chunk boundaries do not show);
//   r = sqrtf(.); a pair's term is r or, WGT, fl(fl(w_i w_j) r), w_N = 1; the 16 terms of a tile are added as a balanced binary
//   tree (index pairs (0,1), (2,3), .. first), separately for the pairs with the observation (A) and the pairs among samples (B),
//   masked and dead pairs entering as +0;
//   a lane adds its tiles k ascending; the 64 lanes of a wave by a butterfly (xor 1, 2, 4, 8, 16, 32); the waves in order;
//   energy = A / N - B / (N D) or, WGT, A - B / D' (fair) or A - B.
// Backward: the same distances; each tile then leaves w = (1 / r or 0 where r == 0) * c in an LDS plane of 16-float blocks
// indexed by t (the lower triangle only), c = 1 / N for a pair with the observation and -1 / (N D) among samples or, WGT,
// fl(w_i w_j) and fl(fl(w_i w_j) * (-1 / D)), 0 for a dead row.  A second pass over the columns gives every row n of a column (row
// N: the observation) g * sum_j w_nj (x_nv - x_jv), j ascending, one fmaf each: lane = (column of the chunk, block of four rows).
// WGT: the rows of a dead sample are staged as zeros in that pass (its NaN must not meet the 0 of its plane entries), and a live
// sample's gradient is g * fmaf(0, -1 / D, s): the same bits while D' > 0, and the 0 / 0 = NaN of the formula where one live
// sample leaves D' = 0.  The writer selects exact zeros for dead rows and unobserved columns.
// LDS at N = 256, backward: 16 640 (chunk) + 2 240 (WGT: weights, marks, D') + 137 280 (plane) = 156 160 B of the 163 840.
// No atomics, no workspace, nothing depends on the grid or on pointer alignment (scalar loads and stores only).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"
#include "snsde_sample_set.h"      // MAX_N, row_of_short, pooled_dims_ok, normalise

namespace {

constexpr int VC = 16;              // columns of a chunk
constexpr int WR = 272;             // floats of a weight row: the 4 R <= 260 staged rows, a multiple of 4
constexpr int META = 16;            // floats behind the two rows: D', P

struct EDims {
    int64_t G, ostride, mstride, V, units;      // ostride = M G S W, mstride = G S W; units = scores = workgroups of work
    int32_t S, W, N, R, RP, T, path;            // R row blocks, RP slab row stride (floats), T = R (R + 1) / 2 tiles
};

struct Col {
    int64_t ys;        // float offset of x_0's component
    int64_t tg;        // float offset of the observation's component in the (outer, G, W) plane
    bool live;         // v < V
};

__device__ __forceinline__ Col col_of(int64_t q, int64_t v, const EDims& d) {
    Col c;
    int64_t o, g, w;
    if (d.path) { o = v / d.W; w = v - o * d.W; g = q; }
    else { o = q / d.G; g = q - o * d.G; w = v; }
    c.live = v < d.V;
    c.ys = o * d.ostride + g * d.S * (int64_t)d.W + w;
    c.tg = (o * d.G + g) * d.W + w;
    return c;
}

// rows of the most populous launch of a bucket, over the rows a pass of the workgroup stages: loads a thread holds for a chunk
constexpr int max_loads(int threads, int tpl) {
    const int rmax = threads == 64 ? 10 : (tpl == 1 ? 22 : (tpl == 3 ? 38 : 65));
    return (4 * rmax + threads / VC - 1) / (threads / VC);
}

// A chunk is staged in two halves, so the loads of the next chunk fly while this one is consumed.  fetch: the thread's column
// (tid & 15) of rows tid >> 4, + THREADS / 16, .. into registers; zeros past V, past row N and - MSK - in every row of an
// unobserved column, of which nothing is read.  Returns whether the column is observed (MSK; else: live).
template <int THREADS, int MAXL, bool MSK>
__device__ __forceinline__ bool fetch(const float* __restrict__ ys, const float* __restrict__ target, const float* __restrict__ mask,
                                      int32_t nan_missing, const Col& cl, const EDims& d, float (&pre)[MAXL]) {
    bool obs = cl.live;
    if constexpr (MSK) {
        if (cl.live) {
            if (mask) obs = mask[cl.tg] != 0.0f;
            else if (nan_missing) {
                const float y = target[cl.tg];
                obs = y == y;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXL; ++i) {
        const int row = (threadIdx.x >> 4) + i * (THREADS / VC);
        float x = 0.0f;
        if (obs) {
            if (row < d.N) x = ys[cl.ys + row_of_short(row, d)];
            else if (row == d.N) x = target[cl.tg];
        }
        pre[i] = x;
    }
    return obs;
}

// put: registers to slab[c][row]; KEEP: a row whose bit of `keep` is clear is staged as zero
template <int THREADS, int MAXL, bool KEEP>
__device__ __forceinline__ void put(const EDims& d, const float (&pre)[MAXL], float* slab, uint32_t keep) {
    const int c = threadIdx.x & (VC - 1);
#pragma unroll
    for (int i = 0; i < MAXL; ++i) {
        const int row = (threadIdx.x >> 4) + i * (THREADS / VC);
        if (row < 4 * d.R) {
            if constexpr (KEEP) slab[c * d.RP + row] = (keep >> i) & 1u ? pre[i] : 0.0f;
            else slab[c * d.RP + row] = pre[i];
        }
    }
}

template <int THREADS, int TPL>
__device__ __forceinline__ void accumulate(const float* slab, const EDims& d, const int (&ri)[TPL], const int (&rj)[TPL],
                                           float (&acc)[TPL][16]) {
    const int kmax = (d.T + THREADS - 1) / THREADS;      // (uniform: rounds of tiles that exist)
#pragma unroll 2
    for (int c = 0; c < VC; ++c) {
        const float* col = slab + c * d.RP;
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
            if (k < kmax) {
                const float4 a4 = *reinterpret_cast<const float4*>(col + ri[k]);
                const float4 b4 = *reinterpret_cast<const float4*>(col + rj[k]);
                const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float df = a[r] - b[s];
                        acc[k][r * 4 + s] = fmaf(df, df, acc[k][r * 4 + s]);
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ float tree16(const float (&e)[16]) {
    float s8[8], s4[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) s8[i] = e[2 * i] + e[2 * i + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) s4[i] = s8[2 * i] + s8[2 * i + 1];
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

enum { LOWER = 0, UPPER = 1, MIXED = 2 };

// s[r] += sum_c w(n_r, j_c) (xn[r] - xj[c]), c ascending; the block of the pair (bn, bj) is stored once, rows = the lower block index
template <int MODE>
__device__ __forceinline__ void block_terms(const float* plane, const float* col, int bn, int bj, const float (&xn)[4], float (&s)[4]) {
    const bool lower = MODE == LOWER || (MODE == MIXED && bj < bn);
    const int t = lower ? bn * (bn + 1) / 2 + bj : bj * (bj + 1) / 2 + bn;
    const float4* blk = reinterpret_cast<const float4*>(plane + t * 16);
    const float4 x4 = *reinterpret_cast<const float4*>(col + 4 * bj);
    const float xj[4] = {x4.x, x4.y, x4.z, x4.w};
    float w[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = blk[i];
        w[i][0] = v.x; w[i][1] = v.y; w[i][2] = v.z; w[i][3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float wt = MODE == LOWER ? w[c][r] : (MODE == UPPER ? w[r][c] : (lower ? w[c][r] : w[r][c]));
            s[r] = fmaf(wt, xn[r] - xj[c], s[r]);
        }
    }
}

// One whole wave: the score's weights and marks into wrow / lrow, row N (the observation) as w = 1 and live, the rows past it, up
// to `rows` (<= N + 4), as dead, and D', P behind the rows
__device__ __forceinline__ void normalise_rows(const float* __restrict__ a, int N, int rows, float* wrow, float* lrow, int lane) {
    const Norm nm = normalise(a, N, wrow, lrow, lane);
    if (lane == 0) {
        wrow[N] = 1.0f;
        lrow[N] = 0.0f;
        lrow[WR] = nm.Dp;
        lrow[WR + 1] = nm.P;
    }
    if (lane >= 1 && N + lane < rows) {
        wrow[N + lane] = 0.0f;
        lrow[N + lane] = __builtin_nanf("");
    }
}

// WGT: the weights of the four rows at r0, and whether each is live
__device__ __forceinline__ void weights4(const float* wrow, int r0, float (&w)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(wrow + r0);
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
}

__device__ __forceinline__ void marks4(const float* lrow, int r0, bool (&l)[4]) {
    const float4 c = *reinterpret_cast<const float4*>(lrow + r0);
    l[0] = c.x == 0.0f; l[1] = c.y == 0.0f; l[2] = c.z == 0.0f; l[3] = c.w == 0.0f;
}

// WGT: the weights and marks of the two row blocks of a tile
__device__ __forceinline__ void tile_weights(const float* wrow, const float* lrow, int ri, int rj, float (&wi)[4], float (&wj)[4],
                                             bool (&li)[4], bool (&lj)[4]) {
    weights4(wrow, ri, wi);
    weights4(wrow, rj, wj);
    marks4(lrow, ri, li);
    marks4(lrow, rj, lj);
}

// waves per SIMD asked of the register allocator: left alone, the weighted forward of three tiles per lane takes 193 VGPRs - two
// waves where the unweighted kernel runs three; held to 168 it needs no scratch
constexpr int min_waves(int tpl, bool bwd, bool wgt) { return tpl == 3 && !bwd && wgt ? 3 : 1; }

template <int THREADS, int TPL, bool BWD, bool WGT, bool MSK>
__global__ void __launch_bounds__(THREADS, min_waves(TPL, BWD, WGT)) snsde_sample_energy_kernel(
    const float* __restrict__ genergy, const float* __restrict__ ys, const float* __restrict__ target, const float* __restrict__ logw,
    const float* __restrict__ mask, EDims d, int32_t D, int32_t fair, int32_t nan_missing, float* __restrict__ energy,
    float* __restrict__ gys, float* __restrict__ gtarget) {
    extern __shared__ float4 lds4[];
    float* slab = reinterpret_cast<float*>(lds4);                  // (VC, RP)
    float* wrow = slab + VC * d.RP;                                // (WR) w_n | (WR) live marks | D', P: WGT only
    float* lrow = wrow + WR;
    float* plane = wrow + (WGT ? 2 * WR + META : 0);               // (T, 4, 4), backward only
    constexpr int WAVES = THREADS / 64, MAXL = max_loads(THREADS, TPL);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid / 64);
    const float fN = (float)d.N, fND = (float)(d.N * D);      // (N D <= 65536: exact)
    int bi[TPL], bj[TPL], ri[TPL], rj[TPL];
    bool have[TPL];
#pragma unroll
    for (int k = 0; k < TPL; ++k) {
        const int t = tid + k * THREADS;
        have[k] = t < d.T;
        int j = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
        while ((j + 1) * (j + 2) / 2 <= t) ++j;
        while (j * (j + 1) / 2 > t) --j;
        bj[k] = have[k] ? j : 0;
        bi[k] = have[k] ? t - j * (j + 1) / 2 : 0;
        ri[k] = 4 * bi[k];
        rj[k] = 4 * bj[k];
    }
    for (int64_t q = blockIdx.x; q < d.units; q += gridDim.x) {
        float acc[TPL][16];
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[k][i] = 0.0f;
        }
        float pre[MAXL];
        bool obs_next = fetch<THREADS, MAXL, MSK>(ys, target, mask, nan_missing, col_of(q, tid & (VC - 1), d), d, pre);
        uint32_t keep = 0u;      // (WGT, backward) bit i: row i of this thread is live or past N
        if constexpr (WGT) {
            __syncthreads();      // (the rows of the last score have been read)
            if (wave == 0) normalise_rows(logw + q * d.N, d.N, 4 * d.R, wrow, lrow, tid);
            __syncthreads();
            if constexpr (BWD) {
#pragma unroll
                for (int i = 0; i < MAXL; ++i) {
                    const int row = (tid >> 4) + i * (THREADS / VC);
                    if (row >= d.N || lrow[row] == 0.0f) keep |= 1u << i;
                }
            }
        }
        for (int64_t v0 = 0; v0 < d.V; v0 += VC) {
            __syncthreads();      // (the last chunk has been read)
            put<THREADS, MAXL, WGT && BWD>(d, pre, slab, keep);
            __syncthreads();
            if (v0 + VC < d.V) fetch<THREADS, MAXL, MSK>(ys, target, mask, nan_missing, col_of(q, v0 + VC + (tid & (VC - 1)), d), d, pre);
            accumulate<THREADS, TPL>(slab, d, ri, rj, acc);
        }
        if (!BWD) {
            float A = 0.0f, B = 0.0f;
#pragma unroll
            for (int k = 0; k < TPL; ++k) {
                float ea[16], eb[16], wi[4], wj[4];
                bool li[4], lj[4];
                if constexpr (WGT) tile_weights(wrow, lrow, ri[k], rj[k], wi, wj, li, lj);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int rowi = ri[k] + r, rowj = rj[k] + s;
                        bool pair = have[k] && rowi < rowj && rowj <= d.N;
                        const float dist = sqrtf(acc[k][r * 4 + s]);
                        float term = dist;
                        if constexpr (WGT) {
                            pair = pair && li[r] && lj[s];
                            term = __fmul_rn(__fmul_rn(wi[r], wj[s]), dist);
                        }
                        ea[r * 4 + s] = pair && rowj == d.N ? term : 0.0f;
                        eb[r * 4 + s] = pair && rowj != d.N ? term : 0.0f;
                    }
                }
                A += tree16(ea);
                B += tree16(eb);
            }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                A += __shfl_xor(A, m, 64);
                B += __shfl_xor(B, m, 64);
            }
            if (WAVES > 1) {
                __syncthreads();      // (every wave is done with the slab: its first words now carry the wave sums)
                if ((tid & 63) == 0) { slab[2 * wave] = A; slab[2 * wave + 1] = B; }
                __syncthreads();
                A = slab[0];
                B = slab[1];
#pragma unroll
                for (int k = 1; k < WAVES; ++k) { A += slab[2 * k]; B += slab[2 * k + 1]; }
            }
            if (tid == 0) {
                if constexpr (WGT) energy[q] = fair ? __fsub_rn(A, __fdiv_rn(B, lrow[WR])) : __fsub_rn(A, B);
                else energy[q] = A / fN - B / fND;
            }
        } else {
            const float cN = 1.0f / fN, cND = -1.0f / fND;
            float cD = 0.0f;      // (WGT) -1 / D
            if constexpr (WGT) cD = fair ? __fdiv_rn(-1.0f, lrow[WR]) : -1.0f;
#pragma unroll
            for (int k = 0; k < TPL; ++k) {
                if (have[k]) {
                    float4* blk = reinterpret_cast<float4*>(plane + (tid + k * THREADS) * 16);
                    float wi[4], wj[4];
                    bool li[4], lj[4];
                    if constexpr (WGT) tile_weights(wrow, lrow, ri[k], rj[k], wi, wj, li, lj);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float w[4];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int rowi = ri[k] + r, rowj = rj[k] + s;
                            const float dist = sqrtf(acc[k][r * 4 + s]);
                            bool pair = rowi != rowj && rowi <= d.N && rowj <= d.N && dist > 0.0f;
                            const bool with_obs = rowi == d.N || rowj == d.N;
                            float coef = with_obs ? cN : cND;      // (one rounding)
                            if constexpr (WGT) {
                                pair = pair && li[r] && lj[s];
                                const float c = __fmul_rn(wi[r], wj[s]);
                                coef = with_obs ? c : __fmul_rn(c, cD);
                            }
                            w[s] = pair ? __fmul_rn(1.0f / dist, coef) : 0.0f;
                        }
                        blk[r] = make_float4(w[0], w[1], w[2], w[3]);
                    }
                }
            }
            const float g = genergy[q];
            const int c = tid & (VC - 1);
            const float* col = slab + c * d.RP;
            Col cl, next = col_of(q, c, d);
            bool obs = true;      // (MSK: the column of cl is observed)
            obs_next = fetch<THREADS, MAXL, MSK>(ys, target, mask, nan_missing, next, d, pre);
            for (int64_t v0 = 0; v0 < d.V; v0 += VC) {
                cl = next;
                if constexpr (MSK) obs = obs_next;
                __syncthreads();      // (the plane is written; the last chunk has been read)
                put<THREADS, MAXL, WGT && BWD>(d, pre, slab, keep);
                __syncthreads();
                if (v0 + VC < d.V) {
                    next = col_of(q, v0 + VC + c, d);
                    obs_next = fetch<THREADS, MAXL, MSK>(ys, target, mask, nan_missing, next, d, pre);
                }
                for (int base = (tid / 64) * 4; base < d.R; base += WAVES * 4) {      // (a wave: four row blocks of the 16 columns)
                    const int bn = min(base + ((tid & 63) >> 4), d.R - 1);
                    const bool own = base + ((tid & 63) >> 4) < d.R;
                    const float4 x4 = *reinterpret_cast<const float4*>(col + 4 * bn);
                    const float xn[4] = {x4.x, x4.y, x4.z, x4.w};
                    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    const int mid = min(base + 4, d.R);
                    for (int j = 0; j < base; ++j) block_terms<LOWER>(plane, col, bn, j, xn, s);
                    for (int j = base; j < mid; ++j) block_terms<MIXED>(plane, col, bn, j, xn, s);
                    for (int j = mid; j < d.R; ++j) block_terms<UPPER>(plane, col, bn, j, xn, s);
                    if (own && cl.live) {
                        bool lv[4];
                        if constexpr (WGT) marks4(lrow, 4 * bn, lv);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * bn + r;
                            if (row < d.N) {
                                float sr = s[r];
                                bool sel = obs;      // (without a mask: true)
                                if constexpr (WGT) {
                                    sr = fmaf(0.0f, cD, s[r]);      // (D' = 0: the formula's 0 / 0)
                                    sel = sel && lv[r];
                                }
                                gys[cl.ys + row_of_short(row, d)] = sel ? __fmul_rn(g, sr) : 0.0f;
                            } else if (row == d.N && gtarget) gtarget[cl.tg] = obs ? __fmul_rn(g, s[r]) : 0.0f;
                        }
                    }
                }
            }
        }
    }
}

bool energy_dims(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t path, EDims* d) {
    int64_t per;
    if (!pooled_dims_ok(outer, members, groups, samples, width, &per)) return false;
    d->G = groups; d->mstride = per; d->ostride = members * per;
    d->S = samples; d->W = width; d->N = members * samples; d->path = path ? 1 : 0;
    d->V = path ? outer * width : width;
    d->units = path ? groups : outer * groups;
    d->R = (d->N + 1 + 3) / 4;
    d->RP = (4 * d->R - 4 + 31) / 32 * 32 + 4;      // >= 4 R, = 4 mod 32: the 16 columns of a 16-byte read fall on 16 different slots
    d->T = d->R * (d->R + 1) / 2;
    return true;
}

struct Args {
    const float *genergy, *ys, *target, *logw, *mask;
    EDims d;
    int32_t D, fair, nan_missing;
    float *energy, *gys, *gtarget;
    hipStream_t stream;
};

// the dims, D and the inputs every entry point fills alike; no weights, no mask: the unweighted call
int fill(Args& a, const float* ys, const float* target, int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
         int32_t fair, int32_t path, void* hip_stream) {
    if (!energy_dims(outer, members, groups, samples, width, path, &a.d)) return SNSDE_ERR_DIMS;
    if (fair && a.d.N < 2) return SNSDE_ERR_DIMS;      // (the unbiased estimator divides by N - 1, or by D' = 0)
    a.genergy = nullptr; a.ys = ys; a.target = target; a.logw = nullptr; a.mask = nullptr;
    a.D = fair ? a.d.N - 1 : a.d.N; a.fair = fair ? 1 : 0; a.nan_missing = 0;
    a.energy = nullptr; a.gys = nullptr; a.gtarget = nullptr;
    a.stream = static_cast<hipStream_t>(hip_stream);
    return SNSDE_OK;
}

template <int THREADS, int TPL, bool BWD, bool WGT, bool MSK>
int launch_as(const Args& a) {
    static SnsdeLdsAttr seen;
    const size_t lds = ((size_t)VC * a.d.RP + (WGT ? 2 * WR + META : 0) + (BWD ? (size_t)a.d.T * 16 : 0)) * sizeof(float);
    auto kernel = snsde_sample_energy_kernel<THREADS, TPL, BWD, WGT, MSK>;
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(kernel), lds, seen);
    if (rc != SNSDE_OK) return rc;
    const unsigned grid = (unsigned)(a.d.units < 8192 ? a.d.units : 8192);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), lds, a.stream, a.genergy, a.ys, a.target, a.logw, a.mask, a.d, a.D, a.fair,
                       a.nan_missing, a.energy, a.gys, a.gtarget);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

template <bool BWD, bool WGT, bool MSK>
int launch_bucket(const Args& a) {
    // (max_loads() holds the largest R of each bucket: 10, 22, 38, 65 row blocks are 55, 253, 741, 2145 tiles)
    if (a.d.T <= 64) return launch_as<64, 1, BWD, WGT, MSK>(a);        // N <= 39
    if (a.d.T <= 256) return launch_as<256, 1, BWD, WGT, MSK>(a);      // N <= 87
    if (a.d.T <= 768) return launch_as<256, 3, BWD, WGT, MSK>(a);      // N <= 151
    return launch_as<256, 9, BWD, WGT, MSK>(a);                        // N <= 256: T <= 2145
}

template <bool BWD>
int launch(const Args& a) {
    const bool msk = a.mask || a.nan_missing;
    if (a.logw) return msk ? launch_bucket<BWD, true, true>(a) : launch_bucket<BWD, true, false>(a);
    return msk ? launch_bucket<BWD, false, true>(a) : launch_bucket<BWD, false, false>(a);
}

}  // namespace

extern "C" int snsde_sample_energy(const float* ys, const float* target, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                   int32_t width, int32_t fair, int32_t path, float* energy, void* hip_stream) {
    if (!ys || !target || !energy) return SNSDE_ERR_NULL;
    Args a;
    const int rc = fill(a, ys, target, outer, members, groups, samples, width, fair, path, hip_stream);
    if (rc != SNSDE_OK) return rc;
    a.energy = energy;
    return launch<false>(a);
}

extern "C" int snsde_sample_energy_backward(const float* grad_energy, const float* ys, const float* target, int64_t outer, int32_t members,
                                            int64_t groups, int32_t samples, int32_t width, int32_t fair, int32_t path, float* grad_ys,
                                            float* grad_target, void* hip_stream) {
    if (!grad_energy || !ys || !target || !grad_ys) return SNSDE_ERR_NULL;
    Args a;
    const int rc = fill(a, ys, target, outer, members, groups, samples, width, fair, path, hip_stream);
    if (rc != SNSDE_OK) return rc;
    a.genergy = grad_energy; a.gys = grad_ys; a.gtarget = grad_target;
    return launch<true>(a);
}

extern "C" int snsde_sample_energy_weighted(const float* ys, const float* target, const float* logw, const float* mask, int64_t outer,
                                            int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t fair, int32_t path,
                                            int32_t nan_missing, float* energy, void* hip_stream) {
    if (!ys || !target || !energy) return SNSDE_ERR_NULL;
    Args a;
    const int rc = fill(a, ys, target, outer, members, groups, samples, width, fair, path, hip_stream);
    if (rc != SNSDE_OK) return rc;
    a.logw = logw; a.mask = mask; a.nan_missing = nan_missing ? 1 : 0; a.energy = energy;
    return launch<false>(a);
}

extern "C" int snsde_sample_energy_weighted_backward(const float* grad_energy, const float* ys, const float* target, const float* logw,
                                                     const float* mask, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                                     int32_t width, int32_t fair, int32_t path, int32_t nan_missing, float* grad_ys,
                                                     float* grad_target, void* hip_stream) {
    if (!grad_energy || !ys || !target || !grad_ys) return SNSDE_ERR_NULL;
    Args a;
    const int rc = fill(a, ys, target, outer, members, groups, samples, width, fair, path, hip_stream);
    if (rc != SNSDE_OK) return rc;
    a.logw = logw; a.mask = mask; a.nan_missing = nan_missing ? 1 : 0;
    a.genergy = grad_energy; a.gys = grad_ys; a.gtarget = grad_target;
    return launch<true>(a);
}
