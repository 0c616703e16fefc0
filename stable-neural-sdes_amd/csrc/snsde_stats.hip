// Mean and unbiased variance over the sample axis of a sampled solve's result, and their adjoint (include/snsde.h: snsde_sample_stats,
// snsde_sample_stats_backward).
// ys is (groups, samples, width); one lane owns one output element (V = 1) or four adjacent ones (V = 4: 16-byte loads and stores,
// width % 4 == 0 and 16-byte aligned pointers) and walks its samples in order, twice: the sum, then the squared deviations from
// the mean.  Adjacent lanes own adjacent columns, so every load of a wave is one contiguous piece of a row.  No atomics, no
// cross-lane traffic and no dependence on the grid: the same bits on every launch.
// snsde_ensemble_stats / snsde_ensemble_stats_backward: the same over the sample paths of a model ensemble, (outer, M, G, S, W) -
// the members' means and variances as above, then the mean, the within-member and the between-member variance across members.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snsde.h"

namespace {

constexpr int ST = 256;      // threads per block

template <int V> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<4> { using T = float4; };

template <int V> __device__ __forceinline__ void load(const float* p, float (&x)[V]) {
    const typename Vec<V>::T v = *reinterpret_cast<const typename Vec<V>::T*>(p);
    if constexpr (V == 4) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
    else x[0] = v;
}
template <int V> __device__ __forceinline__ void store(float* p, const float (&x)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else *p = x[0];
}

template <int V>
__global__ void __launch_bounds__(ST) snsde_sample_stats_kernel(const float* __restrict__ ys, int64_t groups, int32_t S, int32_t W,
                                                                float* __restrict__ mean, float* __restrict__ var) {
    const int64_t wv = W / V, total = groups * wv;      // items: (group, V adjacent columns)
    const float fs = (float)S, fs1 = (float)(S > 1 ? S - 1 : 1);      // (divisions, correctly rounded: one rounding each)
    for (int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST) {
        const int64_t g = e / wv, w = (e - g * wv) * V;
        const float* src = ys + (g * S) * (int64_t)W + w;
        float sum[V], m[V];
#pragma unroll
        for (int i = 0; i < V; ++i) sum[i] = 0.0f;
        for (int s = 0; s < S; ++s) {
            float x[V];
            load<V>(src + (int64_t)s * W, x);
#pragma unroll
            for (int i = 0; i < V; ++i) sum[i] += x[i];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) m[i] = sum[i] / fs;
        store<V>(mean + g * W + w, m);
        if (var) {
            float ss[V];
#pragma unroll
            for (int i = 0; i < V; ++i) ss[i] = 0.0f;
            for (int s = 0; s < S; ++s) {
                float x[V];
                load<V>(src + (int64_t)s * W, x);
#pragma unroll
                for (int i = 0; i < V; ++i) { const float d = x[i] - m[i]; ss[i] = fmaf(d, d, ss[i]); }
            }
#pragma unroll
            for (int i = 0; i < V; ++i) ss[i] /= fs1;
            store<V>(var + g * W + w, ss);
        }
    }
}

// grad_ys[g, s, w] = grad_mean / S + grad_var 2 (ys - mean) / (S - 1): the same ownership as the forward, one walk over s
template <int V>
__global__ void __launch_bounds__(ST) snsde_sample_stats_backward_kernel(const float* __restrict__ gmean, const float* __restrict__ gvar,
                                                                         const float* __restrict__ ys, const float* __restrict__ mean,
                                                                         int64_t groups, int32_t S, int32_t W, float* __restrict__ gys) {
    const int64_t wv = W / V, total = groups * wv;
    const float fs = (float)S, fs1 = (float)(S > 1 ? S - 1 : 1);
    for (int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST) {
        const int64_t g = e / wv, w = (e - g * wv) * V;
        const int64_t row = (g * S) * (int64_t)W + w;
        float a[V], c[V], m[V];
        load<V>(gmean + g * W + w, a);
#pragma unroll
        for (int i = 0; i < V; ++i) { a[i] /= fs; c[i] = 0.0f; m[i] = 0.0f; }
        if (gvar) {
            load<V>(gvar + g * W + w, c);
            load<V>(mean + g * W + w, m);
#pragma unroll
            for (int i = 0; i < V; ++i) c[i] = (2.0f * c[i]) / fs1;
        }
        for (int s = 0; s < S; ++s) {
            float o[V];
            if (gvar) {
                float x[V];
                load<V>(ys + row + (int64_t)s * W, x);
#pragma unroll
                for (int i = 0; i < V; ++i) o[i] = fmaf(c[i], x[i] - m[i], a[i]);
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) o[i] = a[i];
            }
            store<V>(gys + row + (int64_t)s * W, o);
        }
    }
}

// ---- sample paths of a model ensemble (snsde_ensemble_stats): ys is (outer, M, G, S, W), the outputs (outer, G, W) ----------------
// The same ownership: one lane per output element (o, g, w) - or four adjacent w - walks its M members in order and, inside a
// member, its S samples in order, exactly as snsde_sample_stats_kernel walks one group: mean_m and var_m carry its bits.  The
// member means are not kept (M is a run-time count): the pass for `between` forms them again, in the same order, the same bits.

// sum_s x / S of one member's group, s ascending (snsde_sample_stats_kernel's first walk)
template <int V> __device__ __forceinline__ void member_mean(const float* src, int32_t S, int32_t W, float fs, float (&m)[V]) {
    float sum[V];
#pragma unroll
    for (int i = 0; i < V; ++i) sum[i] = 0.0f;
    for (int s = 0; s < S; ++s) {
        float x[V];
        load<V>(src + (int64_t)s * W, x);
#pragma unroll
        for (int i = 0; i < V; ++i) sum[i] += x[i];
    }
#pragma unroll
    for (int i = 0; i < V; ++i) m[i] = sum[i] / fs;
}

template <int V>
__global__ void __launch_bounds__(ST) snsde_ensemble_stats_kernel(const float* __restrict__ ys, int64_t outer, int32_t M, int64_t G, int32_t S,
                                                                  int32_t W, float* __restrict__ mean, float* __restrict__ within,
                                                                  float* __restrict__ between) {
    const int64_t wv = W / V, total = outer * G * wv;      // items: (outer, group, V adjacent columns)
    const int64_t mstride = G * S * (int64_t)W;            // floats from one member's block to the next
    const float fs = (float)S, fs1 = (float)(S > 1 ? S - 1 : 1), fm = (float)M, fm1 = (float)(M > 1 ? M - 1 : 1);
    for (int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST) {
        const int64_t og = e / wv, w = (e - og * wv) * V;
        const int64_t o = og / G, g = og - o * G;
        const float* src0 = ys + o * M * mstride + (g * S) * (int64_t)W + w;      // member 0's group
        const int64_t out = og * W + w;
        float msum[V], wsum[V], mu[V];
#pragma unroll
        for (int i = 0; i < V; ++i) msum[i] = wsum[i] = 0.0f;
        for (int m = 0; m < M; ++m) {
            const float* src = src0 + m * mstride;
            float mm[V];
            member_mean<V>(src, S, W, fs, mm);
#pragma unroll
            for (int i = 0; i < V; ++i) msum[i] += mm[i];
            if (within) {
                float ss[V];
#pragma unroll
                for (int i = 0; i < V; ++i) ss[i] = 0.0f;
                for (int s = 0; s < S; ++s) {
                    float x[V];
                    load<V>(src + (int64_t)s * W, x);
#pragma unroll
                    for (int i = 0; i < V; ++i) { const float d = x[i] - mm[i]; ss[i] = fmaf(d, d, ss[i]); }
                }
#pragma unroll
                for (int i = 0; i < V; ++i) wsum[i] += ss[i] / fs1;
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) { mu[i] = msum[i] / fm; wsum[i] /= fm; }
        if (mean) store<V>(mean + out, mu);
        if (within) store<V>(within + out, wsum);
        if (between) {
            float bs[V];
#pragma unroll
            for (int i = 0; i < V; ++i) bs[i] = 0.0f;
            for (int m = 0; m < M; ++m) {
                float mm[V];
                member_mean<V>(src0 + m * mstride, S, W, fs, mm);
#pragma unroll
                for (int i = 0; i < V; ++i) { const float d = mm[i] - mu[i]; bs[i] = fmaf(d, d, bs[i]); }
            }
#pragma unroll
            for (int i = 0; i < V; ++i) bs[i] /= fm1;
            store<V>(between + out, bs);
        }
    }
}

// grad_ys[o, m, g, s, w] = gmean / (M S) + gwithin 2 (x - mean_m) / ((S - 1) M) + gbetween 2 (mean_m - mean) / ((M - 1) S)
template <int V>
__global__ void __launch_bounds__(ST) snsde_ensemble_stats_backward_kernel(const float* __restrict__ gmean, const float* __restrict__ gwithin,
                                                                           const float* __restrict__ gbetween, const float* __restrict__ ys,
                                                                           int64_t outer, int32_t M, int64_t G, int32_t S, int32_t W,
                                                                           float* __restrict__ gys) {
    const int64_t wv = W / V, total = outer * G * wv;
    const int64_t mstride = G * S * (int64_t)W;
    const float fs = (float)S, fs1 = (float)(S > 1 ? S - 1 : 1), fm = (float)M, fm1 = (float)(M > 1 ? M - 1 : 1);
    for (int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST) {
        const int64_t og = e / wv, w = (e - og * wv) * V;
        const int64_t o = og / G, g = og - o * G;
        const int64_t row0 = o * M * mstride + (g * S) * (int64_t)W + w;
        const int64_t out = og * W + w;
        float a[V], cw[V], cb[V], mu[V];
#pragma unroll
        for (int i = 0; i < V; ++i) a[i] = cw[i] = cb[i] = mu[i] = 0.0f;
        if (gmean) {
            load<V>(gmean + out, a);
#pragma unroll
            for (int i = 0; i < V; ++i) a[i] = (a[i] / fm) / fs;
        }
        if (gwithin) {
            load<V>(gwithin + out, cw);
#pragma unroll
            for (int i = 0; i < V; ++i) cw[i] = ((2.0f * cw[i]) / fs1) / fm;
        }
        if (gbetween) {
            load<V>(gbetween + out, cb);
#pragma unroll
            for (int i = 0; i < V; ++i) cb[i] = ((2.0f * cb[i]) / fm1) / fs;
            float msum[V];
#pragma unroll
            for (int i = 0; i < V; ++i) msum[i] = 0.0f;
            for (int m = 0; m < M; ++m) {
                float mm[V];
                member_mean<V>(ys + row0 + m * mstride, S, W, fs, mm);
#pragma unroll
                for (int i = 0; i < V; ++i) msum[i] += mm[i];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) mu[i] = msum[i] / fm;
        }
        for (int m = 0; m < M; ++m) {
            const int64_t row = row0 + m * mstride;
            float mm[V], base[V];
#pragma unroll
            for (int i = 0; i < V; ++i) { mm[i] = 0.0f; base[i] = a[i]; }
            if (gwithin || gbetween) {
                member_mean<V>(ys + row, S, W, fs, mm);
#pragma unroll
                for (int i = 0; i < V; ++i) base[i] = fmaf(cb[i], mm[i] - mu[i], a[i]);
            }
            for (int s = 0; s < S; ++s) {
                float o_[V];
                if (gwithin) {
                    float x[V];
                    load<V>(ys + row + (int64_t)s * W, x);
#pragma unroll
                    for (int i = 0; i < V; ++i) o_[i] = fmaf(cw[i], x[i] - mm[i], base[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < V; ++i) o_[i] = base[i];
                }
                store<V>(gys + row + (int64_t)s * W, o_);
            }
        }
    }
}

// (outer, M, G, S, W): positive, and the element count fits 63 bits
bool ensemble_dims_ok(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width) {
    if (outer <= 0 || members <= 0 || groups <= 0 || samples <= 0 || width <= 0) return false;
    if (groups > INT64_MAX / samples / width) return false;
    const int64_t per = groups * samples * width;
    return outer <= INT64_MAX / members / per;
}

}  // namespace

extern "C" int snsde_ensemble_stats(const float* ys, int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                    float* mean, float* within, float* between, void* hip_stream) {
    if (!ys) return SNSDE_ERR_NULL;
    if (!ensemble_dims_ok(outer, members, groups, samples, width)) return SNSDE_ERR_DIMS;
    if ((within && samples < 2) || (between && members < 2)) return SNSDE_ERR_DIMS;      // (the unbiased estimates divide by S - 1, M - 1)
    if (!mean && !within && !between) return SNSDE_OK;                                     // (nothing wanted: nothing to launch)
    const bool vec = width % 4 == 0 && ((reinterpret_cast<uintptr_t>(ys) | reinterpret_cast<uintptr_t>(mean) |
                                         reinterpret_cast<uintptr_t>(within) | reinterpret_cast<uintptr_t>(between)) & 15) == 0;
    const int64_t items = outer * groups * (width / (vec ? 4 : 1));
    int64_t blocks = (items + ST - 1) / ST;
    if (blocks > 8192) blocks = 8192;      // (the kernel strides over the rest)
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (vec) hipLaunchKernelGGL(snsde_ensemble_stats_kernel<4>, dim3((unsigned)blocks), dim3(ST), 0, st, ys, outer, members, groups, samples,
                                width, mean, within, between);
    else hipLaunchKernelGGL(snsde_ensemble_stats_kernel<1>, dim3((unsigned)blocks), dim3(ST), 0, st, ys, outer, members, groups, samples,
                            width, mean, within, between);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_ensemble_stats_backward(const float* grad_mean, const float* grad_within, const float* grad_between, const float* ys,
                                             int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                             float* grad_ys, void* hip_stream) {
    if (!grad_ys || ((grad_within || grad_between) && !ys)) return SNSDE_ERR_NULL;
    if (!ensemble_dims_ok(outer, members, groups, samples, width)) return SNSDE_ERR_DIMS;
    if ((grad_within && samples < 2) || (grad_between && members < 2)) return SNSDE_ERR_DIMS;
    uintptr_t al = reinterpret_cast<uintptr_t>(grad_ys) | reinterpret_cast<uintptr_t>(grad_mean) | reinterpret_cast<uintptr_t>(grad_within) |
                   reinterpret_cast<uintptr_t>(grad_between);
    if (grad_within || grad_between) al |= reinterpret_cast<uintptr_t>(ys);
    const bool vec = width % 4 == 0 && (al & 15) == 0;
    const int64_t items = outer * groups * (width / (vec ? 4 : 1));
    int64_t blocks = (items + ST - 1) / ST;
    if (blocks > 8192) blocks = 8192;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (vec) hipLaunchKernelGGL(snsde_ensemble_stats_backward_kernel<4>, dim3((unsigned)blocks), dim3(ST), 0, st, grad_mean, grad_within,
                                grad_between, ys, outer, members, groups, samples, width, grad_ys);
    else hipLaunchKernelGGL(snsde_ensemble_stats_backward_kernel<1>, dim3((unsigned)blocks), dim3(ST), 0, st, grad_mean, grad_within,
                            grad_between, ys, outer, members, groups, samples, width, grad_ys);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_stats_backward(const float* grad_mean, const float* grad_var, const float* ys, const float* mean,
                                           int64_t groups, int32_t samples, int32_t width, float* grad_ys, void* hip_stream) {
    if (!grad_mean || !grad_ys || (grad_var && (!ys || !mean))) return SNSDE_ERR_NULL;
    if (groups <= 0 || samples <= 0 || width <= 0) return SNSDE_ERR_DIMS;
    if (grad_var && samples < 2) return SNSDE_ERR_DIMS;
    if (groups > INT64_MAX / samples / width) return SNSDE_ERR_DIMS;
    uintptr_t al = reinterpret_cast<uintptr_t>(grad_mean) | reinterpret_cast<uintptr_t>(grad_ys);
    if (grad_var) al |= reinterpret_cast<uintptr_t>(grad_var) | reinterpret_cast<uintptr_t>(ys) | reinterpret_cast<uintptr_t>(mean);
    const bool vec = width % 4 == 0 && (al & 15) == 0;
    const int64_t items = groups * (width / (vec ? 4 : 1));
    int64_t blocks = (items + ST - 1) / ST;
    if (blocks > 8192) blocks = 8192;      // (the kernel strides over the rest)
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (vec) hipLaunchKernelGGL(snsde_sample_stats_backward_kernel<4>, dim3((unsigned)blocks), dim3(ST), 0, st, grad_mean, grad_var, ys, mean,
                                groups, samples, width, grad_ys);
    else hipLaunchKernelGGL(snsde_sample_stats_backward_kernel<1>, dim3((unsigned)blocks), dim3(ST), 0, st, grad_mean, grad_var, ys, mean,
                            groups, samples, width, grad_ys);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_stats(const float* ys, int64_t groups, int32_t samples, int32_t width, float* mean, float* var,
                                  void* hip_stream) {
    if (!ys || !mean) return SNSDE_ERR_NULL;
    if (groups <= 0 || samples <= 0 || width <= 0) return SNSDE_ERR_DIMS;
    if (var && samples < 2) return SNSDE_ERR_DIMS;      // (the unbiased variance divides by samples - 1)
    if (groups > INT64_MAX / samples / width) return SNSDE_ERR_DIMS;
    const bool vec = width % 4 == 0 &&
                     ((reinterpret_cast<uintptr_t>(ys) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(var)) & 15) == 0;
    const int64_t items = groups * (width / (vec ? 4 : 1));
    int64_t blocks = (items + ST - 1) / ST;
    if (blocks > 8192) blocks = 8192;      // (the kernel strides over the rest)
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (vec) hipLaunchKernelGGL(snsde_sample_stats_kernel<4>, dim3((unsigned)blocks), dim3(ST), 0, st, ys, groups, samples, width, mean, var);
    else hipLaunchKernelGGL(snsde_sample_stats_kernel<1>, dim3((unsigned)blocks), dim3(ST), 0, st, ys, groups, samples, width, mean, var);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
