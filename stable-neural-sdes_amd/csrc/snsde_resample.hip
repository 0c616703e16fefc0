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

namespace {

constexpr int TH = 256;             // threads of a workgroup
constexpr int MAX_S = 256;          // particles of a group (engine.SCORE_MAX_POOLED)
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

}  // namespace

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
    d.G = groups; d.S = samples; d.W = width; d.stratified = stratified != 0; d.threshold = threshold;
    const int64_t per = (int64_t)samples * width;
    int GP = 1;
    while (2 * GP * samples <= TH && 2 * GP * per <= SLAB_MAX) GP *= 2;
    d.GP = GP;
    d.packs = (groups + GP - 1) / GP;
    const bool vec = width % 4 == 0 && a % 16 == 0 && b % 16 == 0;
    const int pieces = vec ? width / 4 : width;
    int L = 1, lshift = 0;
    while (L < TH && L < pieces) { L *= 2; ++lshift; }
    d.L = L; d.lshift = lshift;
    const unsigned grid = (unsigned)(d.packs < GRID_MAX ? d.packs : GRID_MAX);
    auto kernel = vec ? snsde_sample_resample_kernel<true> : snsde_sample_resample_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), 0, static_cast<hipStream_t>(hip_stream), state, logw, loginc, u, d, state_out,
                       logw_out, ancestor, ess, logz, resampled);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
