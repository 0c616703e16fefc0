// Particle filtering on sample paths: weigh the S paths of a group by the newest observation and resample them, one launch
// (include/snsde.h: snsde_sample_resample).  state is (G, S, W), path n of group g at row g S + n; logw, loginc (G, S);
// u (G) or, stratified, (G, S).  A workgroup of 256 threads takes a pack of GP adjacent groups, GP the largest power of two
// <= max(1, min(256 / S, 4096 / (S W))): thread t = gp S + n is particle n of the pack's group gp, so a pack's weights,
// uniforms and rows are contiguous in memory.  Five phases, LDS between them:
//   weights  thread (gp, n): a_n = logw_n + loginc_n (one rounded addition; loginc NULL: logw_n itself) to LDS.
//   maximum  the thread of particle 0 (the group's leader): mx = max_n a_n, n ascending, and whether an a_n is NaN or +Inf.
//   terms    thread (gp, n): e_n = expf(a_n - mx) to LDS (a group that is all -Inf, or holds a NaN or +Inf, skips to the copy).
//   sums     the leader, n ascending, two sequential chains: P_n = P_{n-1} + e_n (P_{-1} = 0) written over e_n, and
//            q = fmaf(e_n, e_n, q); the first and last n with e_n > 0; then logz = (mx + logf(P_{S-1})) - logf((float)S),
//            ess = (P_{S-1} P_{S-1}) / q and the decision.
//   search   thread (gp, j): t_j = (((float)j + u_j) / (float)S) P_{S-1}, each operation rounded once; ancestor = the number of
//            n < S - 1 with P_n <= t_j by a binary search over the group's P in LDS, clamped to [first, last]; logw_out.
//   rows     all 256 threads: L = min(256, the least power of two >= the 16-byte (or 4-byte) pieces of a row) adjacent lanes
//            copy a row, 256 / L rows at a time, from the ancestor's row to row j.
// The chain makes P non-decreasing whatever the rounding, and P_n == P_{n-1} exactly where e_n == 0: such a particle is never
// counted into, so it is never an ancestor; the clamp to `last` serves t_j rounding up to P_{S-1} behind dead trailing
// particles, the clamp to `first` a u outside [0, 1).  The summation order is a function of S alone (GP, L and the grid only
// say which thread does it).  state is moved as 32-bit or 128-bit words, never computed with: every bit pattern survives.
// No atomics, no workspace, nothing depends on the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"
#include "snsde_sample_set.h"      // MAX_N

namespace {

constexpr int TH = 256;             // threads of a workgroup
constexpr int MAX_S = MAX_N;        // particles of a group
constexpr int SLAB_MAX = 4096;      // floats of state a pack moves at most, where it holds more than one group
constexpr int GRID_MAX = 2048;      // workgroups; the kernel strides over the packs beyond

struct RDims {
    int64_t G, packs;
    int32_t S, W, GP, L, lshift, stratified;
    float threshold;
};

template <bool VEC>
__global__ void __launch_bounds__(TH) snsde_sample_resample_kernel(const float* __restrict__ state, const float* __restrict__ logw,
                                                                   const float* __restrict__ loginc, const float* __restrict__ u,
                                                                   RDims d, float* __restrict__ state_out, float* __restrict__ logw_out,
                                                                   int32_t* __restrict__ ancestor, float* __restrict__ ess,
                                                                   float* __restrict__ logz, int32_t* __restrict__ resampled) {
    __shared__ float sa[TH];         // a_n
    __shared__ float sp[TH];         // e_n, then P_n
    __shared__ int32_t srow[TH];     // the row of the pack that row t is copied from
    __shared__ float smx[TH];        // per group of the pack: the maximum (0 where the group is not summed)
    __shared__ float slz[TH];        // ... logz
    __shared__ int32_t smode[TH];    // ... 0: summed, 1: all -Inf, 2: a NaN or +Inf
    __shared__ int32_t sres[TH];     // ... resampled
    __shared__ int32_t sfirst[TH], slast[TH];      // ... the first and the last particle with e_n > 0
    const int tid = threadIdx.x;
    const int gp = tid / d.S, n = tid - gp * d.S;
    const int tm = tid >> d.lshift, l = tid & (d.L - 1), R = TH >> d.lshift;
    const int pieces = VEC ? d.W >> 2 : d.W;
    const float fS = (float)d.S;
    for (int64_t pack = blockIdx.x; pack < d.packs; pack += gridDim.x) {
        const int64_t g0 = pack * d.GP;
        const int64_t left = d.G - g0;
        const int gpn = (int)(left < d.GP ? left : d.GP);      // groups of this pack
        const bool live = gp < gpn;
        const int64_t at = g0 * d.S + tid;                     // (gi, n) of the (G, S) arrays
        __syncthreads();      // (the last pack has been read)
        if (live) sa[tid] = loginc ? __fadd_rn(logw[at], loginc[at]) : logw[at];
        __syncthreads();
        if (live && n == 0) {
            float mx = -INFINITY;
            bool bad = false;
            for (int k = 0; k < d.S; ++k) {
                const float a = sa[tid + k];
                bad = bad || a != a || a == INFINITY;
                mx = fmaxf(mx, a);
            }
            const int mode = bad ? 2 : mx == -INFINITY ? 1 : 0;
            smode[gp] = mode;
            smx[gp] = mode ? 0.0f : mx;
        }
        __syncthreads();
        if (live && smode[gp] == 0) sp[tid] = expf(sa[tid] - smx[gp]);
        __syncthreads();
        if (live && n == 0) {
            const int64_t gi = g0 + gp;
            const int mode = smode[gp];
            float es = mode == 2 ? NAN : 0.0f, lz = mode == 2 ? NAN : -INFINITY;
            int res = 0, first = 0, last = d.S - 1;
            if (mode == 0) {
                float p = 0.0f, q = 0.0f;
                first = -1;
                for (int k = 0; k < d.S; ++k) {
                    const float e = sp[tid + k];
                    p = __fadd_rn(p, e);
                    q = fmaf(e, e, q);
                    sp[tid + k] = p;
                    if (e > 0.0f) {
                        first = first < 0 ? k : first;
                        last = k;
                    }
                }
                es = __fdiv_rn(__fmul_rn(p, p), q);
                lz = __fsub_rn(__fadd_rn(smx[gp], logf(p)), logf(fS));
                res = d.threshold > 0.0f && (d.threshold >= 1.0f || es < __fmul_rn(d.threshold, fS));
            }
            ess[gi] = es;
            logz[gi] = lz;
            resampled[gi] = res;
            slz[gp] = lz;
            sres[gp] = res;
            sfirst[gp] = first;
            slast[gp] = last;
        }
        __syncthreads();
        if (live) {
            int anc = n;
            float lw = sa[tid];
            if (sres[gp]) {
                const float* P = sp + (tid - n);
                const float uj = d.stratified ? u[at] : u[g0 + gp];
                const float t = __fmul_rn(__fdiv_rn(__fadd_rn((float)n, uj), fS), P[d.S - 1]);
                int lo = 0, hi = d.S - 1;      // the count of P_k <= t among k < S - 1
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (P[mid] <= t) lo = mid + 1; else hi = mid;
                }
                anc = lo < sfirst[gp] ? sfirst[gp] : lo > slast[gp] ? slast[gp] : lo;
                lw = slz[gp];
            }
            ancestor[at] = anc;
            logw_out[at] = lw;
            srow[tid] = tid - n + anc;
        }
        __syncthreads();
        const int rows = gpn * d.S;
        const int64_t base = g0 * d.S * (int64_t)d.W;
#pragma unroll 2
        for (int r = tm; r < rows; r += R) {
            const float* src = state + base + (int64_t)srow[r] * d.W;
            float* dst = state_out + base + (int64_t)r * d.W;
            if (VEC) {
                const float4* s4 = reinterpret_cast<const float4*>(src);
                float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll 2
                for (int c = l; c < pieces; c += d.L) d4[c] = s4[c];
            } else {
#pragma unroll 2
                for (int c = l; c < pieces; c += d.L) dst[c] = src[c];
            }
        }
    }
}

// The adjoint of the step (include/snsde.h: snsde_sample_resample_backward), the forward's pack geometry: thread t = gp S + n is
// particle n of the pack's group gp.  ancestor and resampled are inputs, and with them u and the threshold are constants.  Phases:
//   load     thread (gp, n): a_n as the forward forms it, grad_logw_out[n] (NULL: 0) and ancestor[n] to LDS.
//   maximum  the leader: mx and the group's mode, the forward's loop.  The group counts as resampled where resampled[g] != 0
//            and the mode is 0 (summed); every other group is the identity.
//   terms    thread (gp, n): e_n = expf(a_n - mx) to LDS; in a resampled group, the number of j with ancestor[j] == n (the
//            children of n), j ascending over the group's ancestors in LDS.  An ancestor outside [0, S) equals no n.
//   sums     the leader, n ascending: P = P + e_n (the forward's chain; only P_{S-1} is kept), s = s + grad_logw_out[n], the
//            exclusive prefix of the child counts; c = resampled ? grad_logz + s : grad_logz.
//   weights  thread (gp, n): w_n = e_n / P_{S-1}; z_n = e_n > 0 ? c w_n : 0; grad_a[n] = resampled ? z_n : grad_logw_out[n] + z_n
//            (a group of mode 1 or 2: grad_logw_out[n] itself); in a resampled group, the children of n written behind the
//            prefix in ascending j (a stable fill: thread n alone writes the list of n).
//   rows     the forward's lanes: row n of grad_state is the first child's row of grad_state_out moved, the further children
//            added to it in ascending j, one rounded addition per element; no child: +0; the identity: row n moved.
// Every grad_state_out row has one parent at most, so it is read once, and every grad_state row is written once.  LDS: eleven
// arrays of 256 words (11 KiB, the forward has nine), far below what would limit the 8 workgroups a CU holds by its waves.
template <bool VEC>
__global__ void __launch_bounds__(TH) snsde_sample_resample_backward_kernel(const float* __restrict__ gso, const float* __restrict__ glw,
                                                                            const float* __restrict__ glz, const float* __restrict__ logw,
                                                                            const float* __restrict__ loginc,
                                                                            const int32_t* __restrict__ ancestor,
                                                                            const int32_t* __restrict__ resampled, RDims d,
                                                                            float* __restrict__ gs, float* __restrict__ ga) {
    __shared__ float sa[TH];         // a_n
    __shared__ float sp[TH];         // e_n
    __shared__ float sg[TH];         // grad_logw_out[n]
    __shared__ int32_t sanc[TH];     // ancestor[n]
    __shared__ int32_t scnt[TH];     // the children of row t
    __shared__ int32_t sstart[TH];   // where the list of row t begins in schild (an index of the pack)
    __shared__ int32_t schild[TH];   // the rows of the pack that are children, listed by parent, ascending within a parent
    __shared__ float smx[TH];        // per group of the pack: the maximum
    __shared__ float stot[TH];       // ... P_{S-1}
    __shared__ float sc[TH];         // ... c
    __shared__ int32_t smode[TH];    // ... 0: summed and resampled, 1: summed and kept, 2: all -Inf, a NaN or +Inf
    const int tid = threadIdx.x;
    const int gp = tid / d.S, n = tid - gp * d.S;
    const int tm = tid >> d.lshift, l = tid & (d.L - 1), R = TH >> d.lshift;
    const int pieces = VEC ? d.W >> 2 : d.W;
    for (int64_t pack = blockIdx.x; pack < d.packs; pack += gridDim.x) {
        const int64_t g0 = pack * d.GP;
        const int64_t left = d.G - g0;
        const int gpn = (int)(left < d.GP ? left : d.GP);      // groups of this pack
        const bool live = gp < gpn;
        const int64_t at = g0 * d.S + tid;                     // (gi, n) of the (G, S) arrays
        const int lead = tid - n;                              // the pack row of the group's particle 0
        __syncthreads();      // (the last pack has been read)
        if (live) {
            sa[tid] = loginc ? __fadd_rn(logw[at], loginc[at]) : logw[at];
            sg[tid] = glw ? glw[at] : 0.0f;
            sanc[tid] = ancestor[at];
        }
        __syncthreads();
        if (live && n == 0) {
            float mx = -INFINITY;
            bool bad = false;
            for (int k = 0; k < d.S; ++k) {
                const float a = sa[tid + k];
                bad = bad || a != a || a == INFINITY;
                mx = fmaxf(mx, a);
            }
            const bool summed = !bad && mx != -INFINITY;
            smode[gp] = !summed ? 2 : resampled[g0 + gp] != 0 ? 0 : 1;
            smx[gp] = summed ? mx : 0.0f;
        }
        __syncthreads();
        if (live && smode[gp] != 2) sp[tid] = expf(sa[tid] - smx[gp]);
        if (live && smode[gp] == 0) {
            int cnt = 0;
            for (int j = 0; j < d.S; ++j) cnt += sanc[lead + j] == n;
            scnt[tid] = cnt;
        }
        __syncthreads();
        if (live && n == 0) {
            const int mode = smode[gp];
            const float z = glz ? glz[g0 + gp] : 0.0f;
            float p = 0.0f, s = 0.0f;
            int run = tid;
            if (mode != 2)
                for (int k = 0; k < d.S; ++k) p = __fadd_rn(p, sp[tid + k]);
            if (mode == 0)
                for (int k = 0; k < d.S; ++k) {
                    s = __fadd_rn(s, sg[tid + k]);
                    sstart[tid + k] = run;
                    run += scnt[tid + k];
                }
            stot[gp] = p;
            sc[gp] = mode == 0 ? __fadd_rn(z, s) : z;
        }
        __syncthreads();
        if (live) {
            const int mode = smode[gp];
            float out = sg[tid];
            if (mode != 2) {
                const float e = sp[tid];
                const float zn = e > 0.0f ? __fmul_rn(sc[gp], __fdiv_rn(e, stot[gp])) : 0.0f;
                out = mode == 0 ? zn : __fadd_rn(out, zn);
            }
            ga[at] = out;
            if (mode == 0) {
                int k = sstart[tid];
                for (int j = 0; j < d.S; ++j)
                    if (sanc[lead + j] == n) schild[k++] = lead + j;
            }
        }
        __syncthreads();
        const int rows = gpn * d.S;
        const int64_t base = g0 * d.S * (int64_t)d.W;
        for (int r = tm; r < rows; r += R) {
            const bool res = smode[r / d.S] == 0;
            const int k0 = res ? sstart[r] : 0, kn = !gso ? 0 : res ? scnt[r] : 1;
            float* dst = gs + base + (int64_t)r * d.W;
            if (VEC) {
                float4* d4 = reinterpret_cast<float4*>(dst);
                for (int c = l; c < pieces; c += d.L) {
                    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    for (int k = 0; k < kn; ++k) {
                        const int row = res ? schild[k0 + k] : r;
                        const float4 v = reinterpret_cast<const float4*>(gso + base + (int64_t)row * d.W)[c];
                        if (k == 0) {
                            acc = v;
                        } else {
                            acc.x = __fadd_rn(acc.x, v.x);
                            acc.y = __fadd_rn(acc.y, v.y);
                            acc.z = __fadd_rn(acc.z, v.z);
                            acc.w = __fadd_rn(acc.w, v.w);
                        }
                    }
                    d4[c] = acc;
                }
            } else {
                for (int c = l; c < pieces; c += d.L) {
                    float acc = 0.0f;
                    for (int k = 0; k < kn; ++k) {
                        const float v = gso[base + (int64_t)(res ? schild[k0 + k] : r) * d.W + c];
                        acc = k == 0 ? v : __fadd_rn(acc, v);
                    }
                    dst[c] = acc;
                }
            }
        }
    }
}

// [p, p + np) and [q, q + nq) share a byte (a NULL q shares none)
bool overlaps(const void* p, uint64_t np, const void* q, uint64_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return q && (a < b ? b - a < np : a - b < nq);
}

// The pack and lane geometry of a launch, one statement for the step and for its adjoint: GP groups per workgroup, L lanes per row of
// `vec` ? 16-byte : 4-byte pieces, the packs and the grid.  Returns the grid.
unsigned fill_geometry(RDims& d, int64_t groups, int32_t samples, int32_t width, bool vec) {
    d.G = groups; d.S = samples; d.W = width;
    const int64_t per = (int64_t)samples * width;
    int GP = 1;
    while (2 * GP * samples <= TH && 2 * GP * per <= SLAB_MAX) GP *= 2;
    d.GP = GP;
    d.packs = (groups + GP - 1) / GP;
    const int pieces = vec ? width / 4 : width;
    int L = 1, lshift = 0;
    while (L < TH && L < pieces) { L *= 2; ++lshift; }
    d.L = L; d.lshift = lshift;
    return (unsigned)(d.packs < GRID_MAX ? d.packs : GRID_MAX);
}

}  // namespace

extern "C" int snsde_sample_resample_backward(const float* grad_state_out, const float* grad_logw_out, const float* grad_logz,
                                              const float* logw, const float* loginc, const int32_t* ancestor,
                                              const int32_t* resampled, int64_t groups, int32_t samples, int32_t width,
                                              float* grad_state, float* grad_a, void* hip_stream) {
    if (!logw || !ancestor || !resampled || !grad_state || !grad_a) return SNSDE_ERR_NULL;
    if (groups <= 0 || samples <= 0 || width <= 0 || samples > MAX_S) return SNSDE_ERR_DIMS;
    if (groups > INT64_MAX / samples / width / (int64_t)sizeof(float)) return SNSDE_ERR_DIMS;
    const uint64_t gs_bytes = (uint64_t)groups * samples * sizeof(float), g_bytes = (uint64_t)groups * sizeof(float);
    const uint64_t bytes = gs_bytes * width;
    const struct { const void* p; uint64_t n; } ins[] = {{grad_state_out, bytes}, {grad_logw_out, gs_bytes}, {grad_logz, g_bytes},
                                                         {logw, gs_bytes},        {loginc, gs_bytes},        {ancestor, gs_bytes},
                                                         {resampled, g_bytes}};
    for (const auto& in : ins)      // (an output overlapping an input: rows and weights would be read after they are written)
        if (overlaps(grad_state, bytes, in.p, in.n) || overlaps(grad_a, gs_bytes, in.p, in.n)) return SNSDE_ERR_DIMS;
    if (overlaps(grad_state, bytes, grad_a, gs_bytes)) return SNSDE_ERR_DIMS;
    RDims d;
    d.stratified = 0; d.threshold = 0.0f;
    const bool vec = width % 4 == 0 && reinterpret_cast<uintptr_t>(grad_state_out) % 16 == 0 && reinterpret_cast<uintptr_t>(grad_state) % 16 == 0;
    const unsigned grid = fill_geometry(d, groups, samples, width, vec);
    auto kernel = vec ? snsde_sample_resample_backward_kernel<true> : snsde_sample_resample_backward_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), 0, static_cast<hipStream_t>(hip_stream), grad_state_out, grad_logw_out, grad_logz,
                       logw, loginc, ancestor, resampled, d, grad_state, grad_a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_resample(const float* state, const float* logw, const float* loginc, const float* u, int64_t groups,
                                     int32_t samples, int32_t width, int32_t stratified, float threshold, float* state_out,
                                     float* logw_out, int32_t* ancestor, float* ess, float* logz, int32_t* resampled, void* hip_stream) {
    if (!state || !logw || !u || !state_out || !logw_out || !ancestor || !ess || !logz || !resampled) return SNSDE_ERR_NULL;
    if (groups <= 0 || samples <= 0 || width <= 0 || samples > MAX_S || threshold != threshold) return SNSDE_ERR_DIMS;
    if (groups > INT64_MAX / samples / width / (int64_t)sizeof(float)) return SNSDE_ERR_DIMS;
    const uint64_t bytes = (uint64_t)groups * samples * width * sizeof(float);
    const uintptr_t a = reinterpret_cast<uintptr_t>(state), b = reinterpret_cast<uintptr_t>(state_out);
    if (a < b ? b - a < bytes : a - b < bytes) return SNSDE_ERR_DIMS;      // (state_out overlaps state: rows would be read after they are written)
    RDims d;
    d.stratified = stratified != 0; d.threshold = threshold;
    const bool vec = width % 4 == 0 && a % 16 == 0 && b % 16 == 0;
    const unsigned grid = fill_geometry(d, groups, samples, width, vec);
    auto kernel = vec ? snsde_sample_resample_kernel<true> : snsde_sample_resample_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), 0, static_cast<hipStream_t>(hip_stream), state, logw, loginc, u, d, state_out,
                       logw_out, ancestor, ess, logz, resampled);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
