// Energy score of sample paths against an observation, and its adjoint (include/snsde.h: snsde_sample_energy,
// snsde_sample_energy_backward).
// ys is (outer, M, G, S, W) as in snsde_scores.hip; the pooled sample set of a group g is x_n, n = m S + s, N = M S vectors of V
// components: V = W, one score per (o, g) (path = 0), or V = outer W, component v = o W + w, one score per g (path != 0).  The
// members and outer axes are addressing only.
// Ownership: one workgroup per score.  The N samples and the observation (row N) are the N + 1 rows of one table; rows are taken
// in blocks of four (R = ceil((N + 1) / 4) blocks, the rows past N staged as zeros and masked), and the R (R + 1) / 2 block pairs
// (bi <= bj) - 4 x 4 micro-tiles of row pairs - are dealt to the lanes, tile t = bj (bj + 1) / 2 + bi to lane t mod THREADS.  A
// lane keeps the 16 squared distances of each of its tiles in registers over the whole vector: the columns are consumed in
// chunks of 16, each staged column-major in LDS (slab[c][row], row stride RP = 4 mod 32 words), so a tile reads its two row
// blocks of a column as two 16-byte LDS reads for 16 pairs.  Lanes past V stage zeros and store nothing.  The loads of the next
// chunk are issued into registers before the current one is consumed.
// Buckets by T = R (R + 1) / 2: one wave and one tile per lane (T <= 64: N <= 39), four waves and 1 / 3 / 9 tiles per lane
// (N <= 87 / 151 / 256).
// Summation order (a function of N, V, fair and nothing else):
//   squared distance of a pair: one fmaf(d, d, .) chain over v ascending, d = x_iv - x_jv (chunk boundaries do not show);
//   r = sqrtf(.); the 16 terms of a tile are added as a balanced binary tree (index pairs (0,1), (2,3), .. first), separately
//   for the pairs with the observation (A) and the pairs among samples (B), masked pairs entering as +0;
//   a lane adds its tiles k ascending; the 64 lanes of a wave by a butterfly (xor 1, 2, 4, 8, 16, 32); the waves in order;
//   energy = A / N - B / (N D).
// Backward: the same distances; each tile then leaves w = (1 / r or 0 where r == 0) * (1 / N for a pair with the observation,
// -1 / (N D) among samples) in an LDS plane of 16-float blocks indexed by t (the lower triangle only: 137 KB at N = 256), and a
// second pass over the columns gives every row n of a column (row N: the observation) g * sum_j w_nj (x_nv - x_jv), j ascending,
// one fmaf each: lane = (column of the chunk, block of four rows).  No atomics, nothing depends on the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"

namespace {

constexpr int VC = 16;              // columns of a chunk
constexpr int MAX_N = 256;          // pooled samples (engine.SCORE_MAX_POOLED)

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

__device__ __forceinline__ int64_t row_of(int n, const EDims& d) {
    if (d.S == d.N) return (int64_t)n * d.W;      // (uniform: one member)
    const int m = n / d.S, s = n - m * d.S;
    return m * d.mstride + (int64_t)s * d.W;
}

// rows of the most populous launch of a bucket, over the rows a pass of the workgroup stages: loads a thread holds for a chunk
constexpr int max_loads(int threads, int tpl) {
    const int rmax = threads == 64 ? 10 : (tpl == 1 ? 22 : (tpl == 3 ? 38 : 65));
    return (4 * rmax + threads / VC - 1) / (threads / VC);
}

// A chunk is staged in two halves, so the loads of the next chunk fly while this one is consumed.  fetch: the thread's column
// (tid & 15) of rows tid >> 4, + THREADS / 16, .. into registers, zeros past V and past row N; put: registers to slab[c][row].
template <int THREADS, int MAXL>
__device__ __forceinline__ void fetch(const float* __restrict__ ys, const float* __restrict__ target, const Col& cl, const EDims& d,
                                      float (&pre)[MAXL]) {
#pragma unroll
    for (int i = 0; i < MAXL; ++i) {
        const int row = (threadIdx.x >> 4) + i * (THREADS / VC);
        float x = 0.0f;
        if (cl.live) {
            if (row < d.N) x = ys[cl.ys + row_of(row, d)];
            else if (row == d.N) x = target[cl.tg];
        }
        pre[i] = x;
    }
}

template <int THREADS, int MAXL>
__device__ __forceinline__ void put(const EDims& d, const float (&pre)[MAXL], float* slab) {
    const int c = threadIdx.x & (VC - 1);
#pragma unroll
    for (int i = 0; i < MAXL; ++i) {
        const int row = (threadIdx.x >> 4) + i * (THREADS / VC);
        if (row < 4 * d.R) slab[c * d.RP + row] = pre[i];
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

template <int THREADS, int TPL, bool BWD>
__global__ void __launch_bounds__(THREADS) snsde_sample_energy_kernel(const float* __restrict__ genergy, const float* __restrict__ ys,
                                                                      const float* __restrict__ target, EDims d, int32_t D,
                                                                      float* __restrict__ energy, float* __restrict__ gys,
                                                                      float* __restrict__ gtarget) {
    extern __shared__ float4 lds4[];
    float* slab = reinterpret_cast<float*>(lds4);      // (VC, RP)
    float* plane = slab + VC * d.RP;                   // (T, 4, 4), backward only
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
        fetch<THREADS, MAXL>(ys, target, col_of(q, tid & (VC - 1), d), d, pre);
        for (int64_t v0 = 0; v0 < d.V; v0 += VC) {
            __syncthreads();      // (the last chunk has been read)
            put<THREADS, MAXL>(d, pre, slab);
            __syncthreads();
            if (v0 + VC < d.V) fetch<THREADS, MAXL>(ys, target, col_of(q, v0 + VC + (tid & (VC - 1)), d), d, pre);
            accumulate<THREADS, TPL>(slab, d, ri, rj, acc);
        }
        if (!BWD) {
            float A = 0.0f, B = 0.0f;
#pragma unroll
            for (int k = 0; k < TPL; ++k) {
                float ea[16], eb[16];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int rowi = ri[k] + r, rowj = rj[k] + s;
                        const bool pair = have[k] && rowi < rowj && rowj <= d.N;
                        const float dist = sqrtf(acc[k][r * 4 + s]);
                        ea[r * 4 + s] = pair && rowj == d.N ? dist : 0.0f;
                        eb[r * 4 + s] = pair && rowj != d.N ? dist : 0.0f;
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
            if (tid == 0) energy[q] = A / fN - B / fND;
        } else {
            const float cN = 1.0f / fN, cND = -1.0f / fND;
#pragma unroll
            for (int k = 0; k < TPL; ++k) {
                if (have[k]) {
                    float4* blk = reinterpret_cast<float4*>(plane + (tid + k * THREADS) * 16);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float w[4];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int rowi = ri[k] + r, rowj = rj[k] + s;
                            const float dist = sqrtf(acc[k][r * 4 + s]);
                            const bool pair = rowi != rowj && rowi <= d.N && rowj <= d.N && dist > 0.0f;
                            w[s] = pair ? (1.0f / dist) * ((rowi == d.N || rowj == d.N) ? cN : cND) : 0.0f;
                        }
                        blk[r] = make_float4(w[0], w[1], w[2], w[3]);
                    }
                }
            }
            const float g = genergy[q];
            const int c = tid & (VC - 1);
            const float* col = slab + c * d.RP;
            Col cl, next = col_of(q, c, d);
            fetch<THREADS, MAXL>(ys, target, next, d, pre);
            for (int64_t v0 = 0; v0 < d.V; v0 += VC) {
                cl = next;
                __syncthreads();      // (the plane is written; the last chunk has been read)
                put<THREADS, MAXL>(d, pre, slab);
                __syncthreads();
                if (v0 + VC < d.V) {
                    next = col_of(q, v0 + VC + c, d);
                    fetch<THREADS, MAXL>(ys, target, next, d, pre);
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
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * bn + r;
                            if (row < d.N) gys[cl.ys + row_of(row, d)] = g * s[r];
                            else if (row == d.N && gtarget) gtarget[cl.tg] = g * s[r];
                        }
                    }
                }
            }
        }
    }
}

// (outer, M, G, S, W): positive, the element count fits 63 bits, N = M S within the cap (as snsde_scores.hip: dims_ok)
bool energy_dims(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t path, EDims* d) {
    if (outer <= 0 || members <= 0 || groups <= 0 || samples <= 0 || width <= 0) return false;
    if ((int64_t)members * samples > MAX_N) return false;
    if (groups > INT64_MAX / samples / width) return false;
    const int64_t per = groups * samples * width;
    if (outer > INT64_MAX / members / per) return false;
    d->G = groups; d->mstride = per; d->ostride = members * per;
    d->S = samples; d->W = width; d->N = members * samples; d->path = path ? 1 : 0;
    d->V = path ? outer * width : width;
    d->units = path ? groups : outer * groups;
    d->R = (d->N + 1 + 3) / 4;
    d->RP = (4 * d->R - 4 + 31) / 32 * 32 + 4;      // >= 4 R, = 4 mod 32: the 16 columns of a 16-byte read fall on 16 different slots
    d->T = d->R * (d->R + 1) / 2;
    return true;
}

template <int THREADS, int TPL, bool BWD>
int launch_as(const float* genergy, const float* ys, const float* target, const EDims& d, int32_t D, float* energy, float* gys,
              float* gtarget, hipStream_t stream) {
    static SnsdeLdsAttr seen;
    const size_t lds = ((size_t)VC * d.RP + (BWD ? (size_t)d.T * 16 : 0)) * sizeof(float);
    auto kernel = snsde_sample_energy_kernel<THREADS, TPL, BWD>;
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(kernel), lds, seen);
    if (rc != SNSDE_OK) return rc;
    const unsigned grid = (unsigned)(d.units < 8192 ? d.units : 8192);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), lds, stream, genergy, ys, target, d, D, energy, gys, gtarget);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

template <bool BWD>
int launch(const float* genergy, const float* ys, const float* target, const EDims& d, int32_t D, float* energy, float* gys, float* gtarget,
           void* hip_stream) {
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    // (max_loads() holds the largest R of each bucket: 10, 22, 38, 65 row blocks are 55, 253, 741, 2145 tiles)
    if (d.T <= 64) return launch_as<64, 1, BWD>(genergy, ys, target, d, D, energy, gys, gtarget, stream);        // N <= 39
    if (d.T <= 256) return launch_as<256, 1, BWD>(genergy, ys, target, d, D, energy, gys, gtarget, stream);      // N <= 87
    if (d.T <= 768) return launch_as<256, 3, BWD>(genergy, ys, target, d, D, energy, gys, gtarget, stream);      // N <= 151
    return launch_as<256, 9, BWD>(genergy, ys, target, d, D, energy, gys, gtarget, stream);                      // N <= 256: T <= 2145
}

}  // namespace

extern "C" int snsde_sample_energy(const float* ys, const float* target, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                   int32_t width, int32_t fair, int32_t path, float* energy, void* hip_stream) {
    if (!ys || !target || !energy) return SNSDE_ERR_NULL;
    EDims d;
    if (!energy_dims(outer, members, groups, samples, width, path, &d)) return SNSDE_ERR_DIMS;
    if (fair && d.N < 2) return SNSDE_ERR_DIMS;      // (the unbiased estimator divides by N - 1)
    return launch<false>(nullptr, ys, target, d, fair ? d.N - 1 : d.N, energy, nullptr, nullptr, hip_stream);
}

extern "C" int snsde_sample_energy_backward(const float* grad_energy, const float* ys, const float* target, int64_t outer, int32_t members,
                                            int64_t groups, int32_t samples, int32_t width, int32_t fair, int32_t path, float* grad_ys,
                                            float* grad_target, void* hip_stream) {
    if (!grad_energy || !ys || !target || !grad_ys) return SNSDE_ERR_NULL;
    EDims d;
    if (!energy_dims(outer, members, groups, samples, width, path, &d)) return SNSDE_ERR_DIMS;
    if (fair && d.N < 2) return SNSDE_ERR_DIMS;
    return launch<true>(grad_energy, ys, target, d, fair ? d.N - 1 : d.N, nullptr, grad_ys, grad_target, hip_stream);
}
