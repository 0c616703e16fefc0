// Masked Gaussian log-likelihood of sample paths, its importance-weighted bound, and their adjoint (include/snsde.h:
// snsde_sample_loglik, snsde_sample_loglik_backward).
// ys is (outer, M, G, S, W) as in snsde_energy.hip under path: the pooled sample set of a group g is x_n, n = m S + s, N = M S
// vectors of V = outer W components, v = o W + w, addressed in place; target and mask are (outer, G, W).  An element is observed
// where mask != 0; an unobserved element is selected out: no sample is loaded there, it enters every sum as +0 and its gradient is +0.
// Forward, one workgroup of 256 threads per group.  L = min(32, the largest power of two <= 256 / N) lanes share a sample and a
// chunk is CW = 64 L columns (64 .. 2048): the chunk's residuals d_nv = y_v - x_nv go once from HBM, coalesced along v, into
// the LDS slab (N, RP), RP = CW + (L mod 32) words.  The thread that stages a column holds its y_v and m_v and adds the column's
// residuals as they arrive (n ascending): the sample mean costs no second pass.  Up to CW = 128 the rows of a column are split
// in RS = 256 / CW contiguous parts over as many threads.  The per-sample sums then read the slab transposed: thread
// t = n L + l walks the 64 columns c = l + j L of row n, word n RP + l + j L = t + j L (mod 32): the 32 lanes of a half wave
// fall on 32 different banks (ds_read_b32 banks by 32-lane halves), and the staging writes of a wave are 64 adjacent words.
// Summation order (a function of N and V alone; L, CW and RS follow from N):
//   q_n = sum_v m_v d_nv^2: sub-lane l one chain q = fmaf(m_v * d, d, q) over the columns v = l (mod L) ascending, the L chains
//   by a butterfly (xor 1, 2, .., L / 2); count the same with cnt += m_v;
//   logpx_n = -0.5f * fmaf(inv_var, q_n, (log2pi_f + logvar) * count), divided by count under norm; +0 where count == 0;
//   s_v = sum_n d_nv: n ascending inside each of the RS parts [k N / RS, (k + 1) N / RS), the parts k ascending; e_v = s_v / N;
//   sqerr: thread t one chain fmaf(m_v * e_v, e_v, .) over its columns (v = t mod 256 where CW >= 256, else v = t mod CW for
//   t < CW) ascending, the 64 lanes of a wave by a butterfly (xor 1, .., 32), the four waves in order;
//   bound: a_n = logpx_n + logw_n; max over n; lane i of one wave the chain sum += expf(a_n - max) over n = i (mod 64) ascending,
//   the lanes by a butterfly; max + logf(sum) - logf(N).  A NaN a_n gives NaN; an infinite max gives max - logf(N).
// Backward: a workgroup per (group, 256 adjacent columns); the prologue forms p_n = softmax_n(a_n) and
// c_n = (grad_logpx_n + grad_bound p_n) / (count or 1) * inv_var for the <= 256 samples in LDS (the maximum and the sum by
// butterflies and the waves in order), then a lane walks its own column n ascending.  No atomics, nothing depends on the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"
#include "snsde_loglik_layout.h"      // LDims, col_of, wave_sum_up, loglik_dims (shared with snsde_loglik_noise.hip)

namespace {

// LDS of the forward, in floats: slab (N, RP), mbuf (CW), pbuf (256: the column sums of the parts), abuf (256: a_n), red (4)
__host__ __device__ inline size_t fwd_lds_floats(const LDims& d) { return (size_t)d.N * d.RP + d.CW + 2 * TH + 4; }

// CPT = max(1, CW / 256): columns of a chunk a thread stages
template <int CPT>
__global__ void __launch_bounds__(TH) snsde_sample_loglik_kernel(const float* __restrict__ ys, const float* __restrict__ target,
                                                                 const float* __restrict__ mask, const float* __restrict__ logw, LDims d,
                                                                 float K, float inv_var, float* __restrict__ logpx,
                                                                 float* __restrict__ count, float* __restrict__ bound,
                                                                 float* __restrict__ sqerr) {
    extern __shared__ float lds[];
    float* slab = lds;
    float* mbuf = slab + (size_t)d.N * d.RP;
    float* pbuf = mbuf + d.CW;
    float* abuf = pbuf + TH;
    float* red = abuf + TH;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float fN = (float)d.N;
    // the per-sample sums: thread = (sample sn, sub-lane sl)
    const int sn = tid >> d.lshift, sl = tid & (d.L - 1);
    const bool srole = sn < d.N;
    const float* srow = slab + (srole ? sn : 0) * d.RP + sl;
    // staging and column sums: thread = (column ct [+ 256 i], part k of the rows)
    constexpr int UNR = CPT == 1 ? 8 : 2;
    const int RS = CPT > 1 ? 1 : TH / d.CW;      // (uniform)
    const int ct = CPT > 1 ? tid : (tid & (d.CW - 1)), k = CPT > 1 ? 0 : (tid >> d.cshift);
    const int r0 = k * d.N / RS, r1 = (k + 1) * d.N / RS;
    for (int64_t g = blockIdx.x; g < d.G; g += gridDim.x) {
        float q = 0.0f, cnt = 0.0f, sq = 0.0f;
        // the thread's columns of a chunk: offsets, mask and target, fetched one chunk ahead
        Col cl[CPT];
        float m[CPT], y[CPT];
        auto fetch_cols = [&](int64_t v0) {
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int64_t v = v0 + ct + i * TH;
                cl[i].ys = cl[i].tg = 0;
                m[i] = y[i] = 0.0f;
                if (v < d.V) {
                    cl[i] = col_of(g, v, d);
                    m[i] = mask[cl[i].tg];
                    y[i] = target[cl[i].tg];      // (of an unobserved element: loaded with the mask, selected out below)
                }
            }
        };
        fetch_cols(0);
        for (int64_t v0 = 0; v0 < d.V; v0 += d.CW) {
            __syncthreads();      // (the last chunk has been read)
            bool obs[CPT];
            float s[CPT];
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                obs[i] = m[i] != 0.0f;      // (dead columns and unobserved elements: no sample is loaded)
                s[i] = 0.0f;
                if (k == 0) mbuf[ct + i * TH] = m[i];
            }
#pragma unroll UNR
            for (int n = r0; n < r1; ++n) {
                const int64_t off = row_of_short(n, d);
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const float dd = obs[i] ? y[i] - ys[cl[i].ys + off] : 0.0f;
                    slab[n * d.RP + ct + i * TH] = dd;
                    s[i] += dd;
                }
            }
            if (RS == 1) {
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const float e = s[i] / fN;
                    sq = fmaf(m[i] * e, e, sq);
                }
            } else {
                pbuf[k * d.CW + ct] = s[0];
            }
            __syncthreads();
            if (RS > 1 && k == 0) {
                float s = pbuf[ct];
                for (int j = 1; j < RS; ++j) s += pbuf[j * d.CW + ct];
                const float e = s / fN;
                sq = fmaf(m[0] * e, e, sq);
            }
            if (v0 + d.CW < d.V) fetch_cols(v0 + d.CW);
            if (srole) {
#pragma unroll 8
                for (int j = 0; j < 64; ++j) {
                    const float dd = srow[j * d.L], mm = mbuf[sl + j * d.L];
                    q = fmaf(mm * dd, dd, q);
                    cnt += mm;
                }
            }
        }
        for (int m = 1; m < d.L; m <<= 1) {      // (uniform trip count; the lanes of a sample are adjacent)
            q += __shfl_xor(q, m, 64);
            cnt += __shfl_xor(cnt, m, 64);
        }
        float lp = 0.0f;
        if (cnt != 0.0f) {
            lp = -0.5f * fmaf(inv_var, q, K * cnt);
            if (d.norm) lp = lp / cnt;
        }
        if (srole && sl == 0) {
            const int64_t at = g * d.N + sn;
            logpx[at] = lp;
            abuf[sn] = logw ? lp + logw[at] : lp;
        }
        sq = wave_sum_up(sq);
        if (lane == 0) red[wave] = sq;
        __syncthreads();
        if (wave == 0) {
            float mx = -INFINITY;
            bool bad = false;
            for (int n = lane; n < d.N; n += 64) {
                const float a = abuf[n];
                bad = bad || a != a;
                mx = fmaxf(mx, a);
            }
            mx = wave_max_up(mx);
            bad = __any(bad);
            float r;
            if (bad) {
                r = NAN;
            } else if (isinf(mx)) {
                r = mx - logf(fN);
            } else {
                float sum = 0.0f;
                for (int n = lane; n < d.N; n += 64) sum += expf(abuf[n] - mx);
                sum = wave_sum_up(sum);
                r = mx + logf(sum) - logf(fN);
            }
            if (lane == 0) {
                bound[g] = r;
                count[g] = cnt;      // (thread 0: sample 0, sub-lane 0)
                sqerr[g] = ((red[0] + red[1]) + red[2]) + red[3];
            }
        }
    }
}

__global__ void __launch_bounds__(TH) snsde_sample_loglik_backward_kernel(const float* __restrict__ glogpx, const float* __restrict__ gbound,
                                                                          const float* __restrict__ ys, const float* __restrict__ target,
                                                                          const float* __restrict__ mask, const float* __restrict__ logw,
                                                                          const float* __restrict__ logpx, const float* __restrict__ count,
                                                                          LDims d, float inv_var, float* __restrict__ gys,
                                                                          float* __restrict__ gtarget, float* __restrict__ glogw) {
    __shared__ float cs[MAX_N];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t units = d.G * d.vtiles;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t g = u / d.vtiles, vt = u - g * d.vtiles;
        // prologue: p_n and c_n of the group, thread n
        const bool have = tid < d.N;
        const int64_t at = g * d.N + (have ? tid : 0);
        const float gb = gbound ? gbound[g] : 0.0f;
        float a = -INFINITY, p = 0.0f;
        if (gbound) {      // (uniform: the softmax is needed only by grad_bound)
            if (have) a = logw ? logpx[at] + logw[at] : logpx[at];
            float mx = wave_max_up(a);
            __syncthreads();      // (red of the last unit has been read)
            if (lane == 0) red[wave] = mx;
            __syncthreads();
            mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
            const float ex = have ? expf(a - mx) : 0.0f;
            float sum = wave_sum_up(ex);
            __syncthreads();
            if (lane == 0) red[wave] = sum;
            __syncthreads();
            sum = ((red[0] + red[1]) + red[2]) + red[3];
            p = ex / sum;
        }
        __syncthreads();      // (cs of the last unit has been read)
        if (have) {
            const float gbp = gb * p;
            float c = (glogpx ? glogpx[at] : 0.0f) + gbp;
            if (d.norm) {
                const float cn = count[g];
                c = cn != 0.0f ? c / cn : 0.0f;
            }
            cs[tid] = c * inv_var;
            if (glogw && vt == 0) glogw[at] = gbound ? gbp : 0.0f;
        }
        __syncthreads();
        const int64_t v = vt * TH + tid;
        if (v < d.V) {
            const Col cl = col_of(g, v, d);
            const float m = mask[cl.tg];
            if (m != 0.0f) {
                const float y = target[cl.tg];
                const float* src = ys + cl.ys;
                float* dst = gys + cl.ys;
                float s = 0.0f;
#pragma unroll 8
                for (int n = 0; n < d.N; ++n) {
                    const int64_t r = row_of_short(n, d);
                    const float gr = (cs[n] * m) * (y - src[r]);
                    dst[r] = gr;
                    s += gr;
                }
                if (gtarget) gtarget[cl.tg] = -s;
            } else {
                float* dst = gys + cl.ys;
                for (int n = 0; n < d.N; ++n) dst[row_of_short(n, d)] = 0.0f;
                if (gtarget) gtarget[cl.tg] = 0.0f;
            }
        }
    }
}

bool variance_ok(float logvar, float inv_var) { return isfinite(logvar) && isfinite(inv_var) && inv_var > 0.0f; }

}  // namespace

extern "C" int snsde_sample_loglik(const float* ys, const float* target, const float* mask, const float* logw, int64_t outer,
                                   int32_t members, int64_t groups, int32_t samples, int32_t width, float logvar, float inv_var,
                                   int32_t norm, float* logpx, float* count, float* bound, float* sqerr, void* hip_stream) {
    if (!ys || !target || !mask || !logpx || !count || !bound || !sqerr) return SNSDE_ERR_NULL;
    LDims d;
    if (!loglik_dims(outer, members, groups, samples, width, norm, &d)) return SNSDE_ERR_DIMS;
    if (!variance_ok(logvar, inv_var)) return SNSDE_ERR_DIMS;
    static SnsdeLdsAttr seen[6];      // (by log2 L: the instantiations share entries only where they share a kernel)
    const size_t lds = fwd_lds_floats(d) * sizeof(float);
    auto kernel = d.CW <= TH ? snsde_sample_loglik_kernel<1> : d.CW == 2 * TH ? snsde_sample_loglik_kernel<2>
                : d.CW == 4 * TH ? snsde_sample_loglik_kernel<4> : snsde_sample_loglik_kernel<8>;      // N >= 33, <= 32, <= 16, <= 8
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(kernel), lds, seen[d.lshift]);
    if (rc != SNSDE_OK) return rc;
    const unsigned grid = (unsigned)(d.G < 8192 ? d.G : 8192);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), lds, static_cast<hipStream_t>(hip_stream), ys, target, mask, logw, d,
                       LOG_2PI + logvar, inv_var, logpx, count, bound, sqerr);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_loglik_backward(const float* grad_logpx, const float* grad_bound, const float* ys, const float* target,
                                            const float* mask, const float* logw, const float* logpx, const float* count, int64_t outer,
                                            int32_t members, int64_t groups, int32_t samples, int32_t width, float logvar, float inv_var,
                                            int32_t norm, float* grad_ys, float* grad_target, float* grad_logw, void* hip_stream) {
    if (!ys || !target || !mask || !logpx || !count || !grad_ys) return SNSDE_ERR_NULL;
    LDims d;
    if (!loglik_dims(outer, members, groups, samples, width, norm, &d)) return SNSDE_ERR_DIMS;
    if (!variance_ok(logvar, inv_var)) return SNSDE_ERR_DIMS;
    if (d.vtiles > INT64_MAX / d.G) return SNSDE_ERR_DIMS;
    const int64_t units = d.G * d.vtiles;
    const unsigned grid = (unsigned)(units < 65536 ? units : 65536);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(snsde_sample_loglik_backward_kernel, dim3(grid), dim3(TH), 0, static_cast<hipStream_t>(hip_stream), grad_logpx,
                       grad_bound, ys, target, mask, logw, logpx, count, d, inv_var, grad_ys, grad_target, grad_logw);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
