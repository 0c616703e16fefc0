// What the sample-set kernels share (snsde_scores, snsde_weighted, snsde_energy, snsde_loglik, snsde_classify, snsde_resample):
// device and host helpers, no kernels.  The pooled layout: ys is (outer, M, G, S, W); the sample set of a group g is x_n,
// n = m S + s, N = M S <= MAX_N of them; the members axis is addressing only (member stride G S W), so a pooled call and the
// members = 1 call on the permuted (outer G, M S, W) tensor run the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int MAX_N = 256;          // pooled samples a kernel stages on chip (engine.SCORE_MAX_POOLED)
constexpr int LANES = 64;

// float offset of x_n from x_0 in one column: rows of W floats, members mstride floats apart
__device__ __forceinline__ int64_t pooled_row(int n, int S, int W, int64_t mstride) {
    const int m = n / S, s = n - m * S;
    return m * mstride + (int64_t)s * W;
}

// ... of a dims struct that carries S, W, mstride
template <class D>
__device__ __forceinline__ int64_t row_of(int n, const D& d) {
    return pooled_row(n, d.S, d.W, d.mstride);
}

// ... and N: one member takes a branch (uniform) around the division
template <class D>
__device__ __forceinline__ int64_t row_of_short(int n, const D& d) {
    if (d.S == d.N) return (int64_t)n * d.W;
    return pooled_row(n, d.S, d.W, d.mstride);
}

// (outer, M, G, S, W): positive, N = M S within the cap, the element count fits 63 bits; per = G S W
inline bool pooled_dims_ok(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int64_t* per) {
    if (outer <= 0 || members <= 0 || groups <= 0 || samples <= 0 || width <= 0) return false;
    if ((int64_t)members * samples > MAX_N) return false;
    if (groups > INT64_MAX / samples / width) return false;
    *per = groups * samples * width;
    return outer <= INT64_MAX / members / *per;
}

__device__ __forceinline__ float sign0(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// v_l <- v_l + v_(l xor s), s = 32, 16, 8, 4, 2, 1: every lane ends with the same bits (the addition commutes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = __fadd_rn(v, __shfl_xor(v, s, LANES));
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, LANES));
    return v;
}

// ---- weights -----------------------------------------------------------------------------------------------------------------
struct Norm {
    float Dp;      // D' = sum_n w_n (1 - w_n)
    float P;       // sum_n e_n (NaN: an unusable weight set)
    int F;         // live samples
};

// One whole wave normalises the N log-weights at `a` into wrow (w_n) and lrow (0 live / NaN dead: added to a sample it
// leaves a live one as it is and makes a dead one compare with nobody); every lane returns the same Norm.  Lane l holds a_n for
// n = l, 64 + l, 128 + l, 192 + l (-Inf past N).
//   mx = fmaxf over all a_n;  e_n = expf(a_n - mx), the difference rounded once
//   P  = ((T_0 + T_1) + T_2) + T_3,  T_i = the butterfly wave_sum of e_(64 i + l) over the lanes l, zeros past N
//   w_n = e_n / P;  D' by the same tree over t_n = w_n (1 - w_n), each of the two operations rounded once
// A sample is dead where e_n == 0 and P is a number.  Where P is NaN (all -Inf, a NaN or a +Inf weight) every w_n is NaN, 0 / NaN
// included, and nothing is dead.
__device__ __forceinline__ Norm normalise(const float* __restrict__ a, int N, float* wrow, float* lrow, int lane) {
    float av[4], e[4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = i * LANES + lane;
        av[i] = n < N ? a[n] : -INFINITY;
        mx = fmaxf(mx, av[i]);
    }
    mx = wave_max(mx);
    float T[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[i] = i * LANES + lane < N ? expf(__fsub_rn(av[i], mx)) : 0.0f;
        T[i] = wave_sum(e[i]);
    }
    Norm r;
    r.P = __fadd_rn(__fadd_rn(__fadd_rn(T[0], T[1]), T[2]), T[3]);
    r.F = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = i * LANES + lane;
        const float w = __fdiv_rn(e[i], r.P);
        const bool alive = n < N && !(e[i] == 0.0f && r.P == r.P);
        r.F += __popcll(__ballot(alive));
        T[i] = wave_sum(n < N ? __fmul_rn(w, __fsub_rn(1.0f, w)) : 0.0f);
        if (n < N) {
            wrow[n] = w;
            lrow[n] = alive ? 0.0f : __builtin_nanf("");
        }
    }
    r.Dp = __fadd_rn(__fadd_rn(__fadd_rn(T[0], T[1]), T[2]), T[3]);
    return r;
}

// ---- the column tiles of the score kernels (snsde_scores.hip, snsde_weighted.hip) --------------------------------------------
// A workgroup of four waves takes one tile (o, g, 64 adjacent columns) and stages its (N, 64) slab in LDS, row-major: lane j
// reads bank j of every row.
constexpr int ST = 256;             // threads per block
constexpr int WAVES = ST / LANES;   // waves sharing a tile

struct Dims {
    int64_t outer, G, mstride, wtiles, tiles;      // mstride = G S W; tiles = outer G wtiles, wtiles = ceil(W / 64)
    int32_t M, S, W, N;
};

struct Tile {
    int64_t og;        // o G + g
    int64_t base;      // float offset of x_0 of this lane's column
    int64_t out;       // float offset of this lane's element in an (outer, G, W) plane
    bool live;         // column < W (lanes of the tail tile are guarded, not clamped)
};

__device__ __forceinline__ Tile tile_of(int64_t t, const Dims& d, int lane) {
    Tile r;
    r.og = t / d.wtiles;
    const int col = (int)(t - r.og * d.wtiles) * LANES + lane;
    const int64_t o = r.og / d.G, g = r.og - o * d.G;
    r.live = col < d.W;
    r.base = o * d.M * d.mstride + (g * d.S) * (int64_t)d.W + col;
    r.out = r.og * d.W + col;
    return r;
}

// the waves of the block stage the slab: wave k rows k, k + 4, ..; dead lanes hold zeros
__device__ __forceinline__ void stage(const float* __restrict__ ys, const Tile& t, const Dims& d, float* slab, int wave, int lane) {
    for (int n = wave; n < d.N; n += WAVES) slab[n * LANES + lane] = t.live ? ys[t.base + row_of(n, d)] : 0.0f;
}

inline bool dims_ok(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, Dims* d) {
    if (!pooled_dims_ok(outer, members, groups, samples, width, &d->mstride)) return false;
    d->outer = outer; d->G = groups;
    d->M = members; d->S = samples; d->W = width; d->N = members * samples;
    d->wtiles = ((int64_t)width + LANES - 1) / LANES;
    d->tiles = outer * groups * d->wtiles;      // (<= outer G W)
    return true;
}

}  // namespace
