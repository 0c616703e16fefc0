// Masked Gaussian log-likelihood of sample paths under a log-std per channel or per entry, its importance-weighted bound and their
// adjoint, the log-std included (include/snsde.h: snsde_sample_loglik_noise, _noise_backward, _noise_reduce).  The sibling of
// snsde_loglik.hip (one scalar variance): the same layout, decomposition and L / CW / RS scheme (snsde_loglik_layout.h), read its
// head comment first.  log_std is (W) in channel mode - column v = o W + w reads entry w - or the (outer, G, W) plane of target and
// mask in entry mode; the mode is a compile-time variant.  ls_v is loaded only where m_v != 0: at an unobserved element it reaches
// no sum and its gradient is an exact +0.
// Forward: the thread that stages a column holds y_v, m_v and, where observed, ls_v, and forms once per column
//   iv_v = expf(-2.0f * ls_v),  u_v = m_v * iv_v,  t_v = m_v * fmaf(2.0f, ls_v, log2pi_f)        (u_v = t_v = +0 where unobserved)
// into the LDS rows ubuf, tbuf next to mbuf (CW words each, read at the same word index as mbuf: a broadcast per sample, the bank
// pattern of the slab read unchanged).  LDS: slab (N, RP) + 3 CW + 2 * 256 + 6 words: 92,184 bytes at N = 8 (CW = 2048, the
// most: one workgroup per CU where the scalar kernel fits two), 80,920 at N = 16, 74,776 at N = 32, 69,400 at N = 256.
// Summation order (a function of N and V alone):
//   q_n = sum_v u_v d_nv^2: sub-lane l one chain q = fmaf(u_v * d, d, q) over the columns v = l (mod L) ascending, the L chains
//   by a butterfly (xor 1, 2, .., L / 2);
//   count = sum_v m_v and lv = sum_v t_v: the same chains and butterfly (cnt += m_v, lv += t_v), formed by the sub-lanes of
//   sample 0 and handed to the workgroup through LDS: count has the bits of snsde_sample_loglik;
//   logpx_n = -0.5f * (q_n + lv), divided by count under norm; +0 where count == 0;
//   s_v, e_v, sqerr and bound: as in snsde_loglik.hip.
// Backward: a workgroup per (group, 256 adjacent columns); the prologue forms p_n = softmax_n(a_n) and
// c_n = (grad_logpx_n + grad_bound p_n) / (count or 1) in LDS as the scalar kernel does (without its inv_var factor), then the
// lane that owns a column walks n ascending:
//   grad_ys[n, v] = (c_n * u_v) * d_nv;  grad_target[v] = -sum_n grad_ys[n, v];
//   grad_log_std[v] = m_v * r,  r the chain r = fmaf(c_n, fmaf(d * iv_v, d, -1.0f), r);  +0 where unobserved.
// grad_log_std is always the per-entry plane (outer, G, W).  The per-channel gradient is its column sum over the outer G rows,
// snsde_sample_loglik_noise_reduce: stage 1, workgroup k sums rows [64 k, 64 (k + 1)) ascending per column into row k of the
// caller's partial plane; stage 2 sums the rows of that plane ascending.  rows <= 64: stage 1 writes the result itself.
// No atomics, nothing depends on the grid or on alignment.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"
#include "snsde_loglik_layout.h"      // LDims, col_of, channel_of, wave_sum_up, loglik_dims

namespace {

constexpr int RR = SNSDE_LOGLIK_NOISE_REDUCE_ROWS;      // rows a stage-1 workgroup sums

// LDS of the forward, in floats: slab (N, RP), mbuf, ubuf, tbuf (CW each), pbuf (256), abuf (256), red (4), cl (2: count, lv)
__host__ __device__ inline size_t noise_lds_floats(const LDims& d) { return (size_t)d.N * d.RP + 3 * (size_t)d.CW + 2 * TH + 6; }

// CPT = max(1, CW / 256): columns of a chunk a thread stages; ENTRY: log_std is the (outer, G, W) plane, else (W)
template <int CPT, bool ENTRY>
__global__ void __launch_bounds__(TH) snsde_sample_loglik_noise_kernel(const float* __restrict__ ys, const float* __restrict__ target,
                                                                       const float* __restrict__ mask, const float* __restrict__ logw,
                                                                       const float* __restrict__ lstd, LDims d, float* __restrict__ logpx,
                                                                       float* __restrict__ count, float* __restrict__ bound,
                                                                       float* __restrict__ sqerr) {
    extern __shared__ float lds[];
    float* slab = lds;
    float* mbuf = slab + (size_t)d.N * d.RP;
    float* ubuf = mbuf + d.CW;
    float* tbuf = ubuf + d.CW;
    float* pbuf = tbuf + d.CW;
    float* abuf = pbuf + TH;
    float* red = abuf + TH;
    float* cl2 = red + 4;
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
        float q = 0.0f, cnt = 0.0f, lv = 0.0f, sq = 0.0f;
        // the thread's columns of a chunk: offsets, mask, target and log-std, fetched one chunk ahead
        Col cl[CPT];
        float m[CPT], y[CPT], ls[CPT];
        auto fetch_cols = [&](int64_t v0) {
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int64_t v = v0 + ct + i * TH;
                cl[i].ys = cl[i].tg = 0;
                m[i] = y[i] = ls[i] = 0.0f;
                if (v < d.V) {
                    cl[i] = col_of(g, v, d);
                    m[i] = mask[cl[i].tg];
                    y[i] = target[cl[i].tg];      // (of an unobserved element: loaded with the mask, selected out below)
                    if (m[i] != 0.0f) ls[i] = lstd[ENTRY ? cl[i].tg : channel_of(v, d)];
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
                if (k == 0) {
                    const float iv = expf(-2.0f * ls[i]);
                    mbuf[ct + i * TH] = m[i];
                    ubuf[ct + i * TH] = obs[i] ? m[i] * iv : 0.0f;
                    tbuf[ct + i * TH] = obs[i] ? m[i] * fmaf(2.0f, ls[i], LOG_2PI) : 0.0f;
                }
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
                    const float dd = srow[j * d.L], uu = ubuf[sl + j * d.L];
                    q = fmaf(uu * dd, dd, q);
                }
            }
            if (wave == 0) {      // (sample 0 lives in wave 0: L <= 32; the sample-independent chains once per workgroup)
#pragma unroll 8
                for (int j = 0; j < 64; ++j) {
                    cnt += mbuf[sl + j * d.L];
                    lv += tbuf[sl + j * d.L];
                }
            }
        }
        for (int m = 1; m < d.L; m <<= 1) {      // (uniform trip count; the lanes of a sample are adjacent)
            q += __shfl_xor(q, m, 64);
            cnt += __shfl_xor(cnt, m, 64);
            lv += __shfl_xor(lv, m, 64);
        }
        if (tid == 0) {
            cl2[0] = cnt;
            cl2[1] = lv;
        }
        __syncthreads();
        cnt = cl2[0];
        lv = cl2[1];
        float lp = 0.0f;
        if (cnt != 0.0f) {
            lp = -0.5f * (q + lv);
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
                count[g] = cnt;
                sqerr[g] = ((red[0] + red[1]) + red[2]) + red[3];
            }
        }
    }
}

template <bool ENTRY>
__global__ void __launch_bounds__(TH) snsde_sample_loglik_noise_backward_kernel(
    const float* __restrict__ glogpx, const float* __restrict__ gbound, const float* __restrict__ ys, const float* __restrict__ target,
    const float* __restrict__ mask, const float* __restrict__ logw, const float* __restrict__ lstd, const float* __restrict__ logpx,
    const float* __restrict__ count, LDims d, float* __restrict__ gys, float* __restrict__ gtarget, float* __restrict__ glogw,
    float* __restrict__ glstd) {
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
            cs[tid] = c;
            if (glogw && vt == 0) glogw[at] = gbound ? gbp : 0.0f;
        }
        __syncthreads();
        const int64_t v = vt * TH + tid;
        if (v < d.V) {
            const Col cl = col_of(g, v, d);
            const float m = mask[cl.tg];
            if (m != 0.0f) {
                const float y = target[cl.tg];
                const float iv = expf(-2.0f * lstd[ENTRY ? cl.tg : channel_of(v, d)]);
                const float uu = m * iv;
                const float* src = ys + cl.ys;
                float* dst = gys + cl.ys;
                float s = 0.0f, r = 0.0f;
#pragma unroll 8
                for (int n = 0; n < d.N; ++n) {
                    const int64_t ro = row_of_short(n, d);
                    const float c = cs[n], dd = y - src[ro];
                    const float gr = (c * uu) * dd;
                    dst[ro] = gr;
                    s += gr;
                    r = fmaf(c, fmaf(dd * iv, dd, -1.0f), r);
                }
                if (gtarget) gtarget[cl.tg] = -s;
                if (glstd) glstd[cl.tg] = m * r;
            } else {
                float* dst = gys + cl.ys;
                for (int n = 0; n < d.N; ++n) dst[row_of_short(n, d)] = 0.0f;
                if (gtarget) gtarget[cl.tg] = 0.0f;
                if (glstd) glstd[cl.tg] = 0.0f;
            }
        }
    }
}

// out[k, w] = sum of in[r, w] over r in [k per, min(rows, (k + 1) per)) ascending; grid (ceil(W / 256), row blocks)
__global__ void __launch_bounds__(TH) snsde_sample_loglik_noise_reduce_kernel(const float* __restrict__ in, int64_t rows, int32_t W,
                                                                              int64_t per, float* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * TH + threadIdx.x;
    if (w >= W) return;
    for (int64_t k = blockIdx.y; k * per < rows; k += gridDim.y) {
        const int64_t r0 = k * per, r1 = r0 + per < rows ? r0 + per : rows;
        float s = in[r0 * W + w];
        for (int64_t r = r0 + 1; r < r1; ++r) s += in[r * W + w];
        out[k * W + w] = s;
    }
}

bool mode_ok(int32_t noise_mode) { return noise_mode == SNSDE_NOISE_CHANNEL || noise_mode == SNSDE_NOISE_ENTRY; }

template <bool ENTRY>
int launch_forward(const float* ys, const float* target, const float* mask, const float* logw, const float* lstd, const LDims& d,
                   float* logpx, float* count, float* bound, float* sqerr, hipStream_t stream) {
    static SnsdeLdsAttr seen[4];      // (one per kernel, by CPT bucket: a kernel's limit is only ever raised)
    const size_t lds = noise_lds_floats(d) * sizeof(float);
    auto kernel = d.CW <= TH       ? snsde_sample_loglik_noise_kernel<1, ENTRY>
                  : d.CW == 2 * TH ? snsde_sample_loglik_noise_kernel<2, ENTRY>
                  : d.CW == 4 * TH ? snsde_sample_loglik_noise_kernel<4, ENTRY>
                                   : snsde_sample_loglik_noise_kernel<8, ENTRY>;      // N >= 33, <= 32, <= 16, <= 8
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(kernel), lds, seen[d.cshift > 8 ? d.cshift - 8 : 0]);
    if (rc != SNSDE_OK) return rc;
    const unsigned grid = (unsigned)(d.G < 8192 ? d.G : 8192);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), lds, stream, ys, target, mask, logw, lstd, d, logpx, count, bound, sqerr);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

}  // namespace

extern "C" int snsde_sample_loglik_noise(const float* ys, const float* target, const float* mask, const float* logw,
                                         const float* log_std, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                         int32_t width, int32_t noise_mode, int32_t norm, float* logpx, float* count, float* bound,
                                         float* sqerr, void* hip_stream) {
    if (!ys || !target || !mask || !log_std || !logpx || !count || !bound || !sqerr) return SNSDE_ERR_NULL;
    LDims d;
    if (!loglik_dims(outer, members, groups, samples, width, norm, &d) || !mode_ok(noise_mode)) return SNSDE_ERR_DIMS;
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    return noise_mode == SNSDE_NOISE_ENTRY ? launch_forward<true>(ys, target, mask, logw, log_std, d, logpx, count, bound, sqerr, stream)
                                           : launch_forward<false>(ys, target, mask, logw, log_std, d, logpx, count, bound, sqerr, stream);
}

extern "C" int snsde_sample_loglik_noise_backward(const float* grad_logpx, const float* grad_bound, const float* ys, const float* target,
                                                  const float* mask, const float* logw, const float* log_std, const float* logpx,
                                                  const float* count, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                                  int32_t width, int32_t noise_mode, int32_t norm, float* grad_ys, float* grad_target,
                                                  float* grad_logw, float* grad_log_std, void* hip_stream) {
    if (!ys || !target || !mask || !log_std || !logpx || !count || !grad_ys) return SNSDE_ERR_NULL;
    LDims d;
    if (!loglik_dims(outer, members, groups, samples, width, norm, &d) || !mode_ok(noise_mode)) return SNSDE_ERR_DIMS;
    if (d.vtiles > INT64_MAX / d.G) return SNSDE_ERR_DIMS;
    const int64_t units = d.G * d.vtiles;
    const unsigned grid = (unsigned)(units < 65536 ? units : 65536);      // (the kernel strides over the rest)
    auto kernel = noise_mode == SNSDE_NOISE_ENTRY ? snsde_sample_loglik_noise_backward_kernel<true>
                                                  : snsde_sample_loglik_noise_backward_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), 0, static_cast<hipStream_t>(hip_stream), grad_logpx, grad_bound, ys, target, mask,
                       logw, log_std, logpx, count, d, grad_ys, grad_target, grad_logw, grad_log_std);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_loglik_noise_reduce(const float* grad_entry, int64_t rows, int32_t width, float* partial,
                                                float* grad_channel, void* hip_stream) {
    if (!grad_entry || !grad_channel) return SNSDE_ERR_NULL;
    if (rows <= 0 || width <= 0 || rows > INT64_MAX / width) return SNSDE_ERR_DIMS;
    const int64_t parts = (rows + RR - 1) / RR;
    if (parts > 1 && !partial) return SNSDE_ERR_NULL;
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const unsigned gx = (unsigned)((width + TH - 1) / TH);
    const unsigned gy = (unsigned)(parts < 32768 ? parts : 32768);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(snsde_sample_loglik_noise_reduce_kernel, dim3(gx, gy), dim3(TH), 0, stream, grad_entry, rows, width, (int64_t)RR,
                       parts > 1 ? partial : grad_channel);
    if (hipGetLastError() != hipSuccess) return SNSDE_ERR_LAUNCH;
    if (parts > 1) {
        hipLaunchKernelGGL(snsde_sample_loglik_noise_reduce_kernel, dim3(gx, 1), dim3(TH), 0, stream, partial, parts, width, parts,
                           grad_channel);
        if (hipGetLastError() != hipSuccess) return SNSDE_ERR_LAUNCH;
    }
    return SNSDE_OK;
}
