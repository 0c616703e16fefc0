// What the two likelihood modules share (snsde_loglik.hip: one scalar variance; snsde_loglik_noise.hip: a log-std per channel or
// per entry): the dims record with the L / CW / RP scheme, the column addressing and the ascending butterflies.  No kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde_sample_set.h"      // MAX_N, row_of_short, pooled_dims_ok

namespace {

constexpr int TH = 256;             // threads of a workgroup
constexpr int MAX_L = 32;           // lanes per sample
constexpr float LOG_2PI = 1.8378770664093453f;

struct LDims {
    int64_t G, ostride, mstride, V, vtiles;      // ostride = M G S W, mstride = G S W; vtiles = ceil(V / 256) (backward)
    int32_t S, W, N, L, lshift, CW, cshift, RP, norm, outer1;
};

struct Col {
    int64_t ys;        // float offset of x_0's component
    int64_t tg;        // float offset of the component in the (outer, G, W) planes
};

__device__ __forceinline__ Col col_of(int64_t g, int64_t v, const LDims& d) {
    int64_t o = 0, w = v;
    if (!d.outer1) {
        if (d.V <= INT32_MAX) {      // (uniform)
            const uint32_t o32 = (uint32_t)v / (uint32_t)d.W;
            o = o32;
            w = (uint32_t)v - o32 * (uint32_t)d.W;
        } else {
            o = v / d.W;
            w = v - o * d.W;
        }
    }
    Col c;
    c.ys = o * d.ostride + g * d.S * (int64_t)d.W + w;
    c.tg = (o * d.G + g) * d.W + w;
    return c;
}

// the channel w = v mod W of column v (what col_of divides by: one division after inlining)
__device__ __forceinline__ int64_t channel_of(int64_t v, const LDims& d) {
    if (d.outer1) return v;
    if (d.V <= INT32_MAX) return (uint32_t)v % (uint32_t)d.W;      // (uniform)
    return v % d.W;
}

// The butterflies of the likelihood run xor 1, 2, .., 32 (its summation order), those of snsde_sample_set.h 32, .., 1: other bits
__device__ __forceinline__ float wave_sum_up(float x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

__device__ __forceinline__ float wave_max_up(float x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
    return x;
}

inline bool loglik_dims(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t norm, LDims* d) {
    int64_t per;
    if (!pooled_dims_ok(outer, members, groups, samples, width, &per)) return false;
    d->G = groups; d->mstride = per; d->ostride = members * per;
    d->S = samples; d->W = width; d->N = members * samples; d->norm = norm ? 1 : 0;
    d->V = outer * width;
    d->vtiles = (d->V + TH - 1) / TH;
    d->outer1 = outer == 1;
    int L = 1, ls = 0;
    while (2 * L <= MAX_L && 2 * L * d->N <= TH) { L *= 2; ++ls; }
    d->L = L; d->lshift = ls;
    d->CW = 64 * L; d->cshift = 6 + ls;
    d->RP = d->CW + (L & 31);
    return true;
}

}  // namespace
