// Classification with sample paths: the predictive (model-average) negative log-likelihood of a label, the expected
// cross-entropy, the predictive distribution with its entropy split, and their adjoint (include/snsde.h: snsde_sample_class,
// snsde_sample_class_backward).
// logits is (outer, M, G, S, C) as ys in snsde_scores.hip: the pooled path of group (o, g) is n = m S + s, N = M S <= 256 rows of C
// stored floats, addressed in place.  binary: C = 1 stored, the two class logits of a path are (0, z).  A workgroup of 256
// threads takes a pack of GP adjacent groups (their GP N rows), in four phases:
//   stage   where the pack's slab of GP N C floats is at most 24576 (96 KiB) it goes once from memory into LDS, all threads,
//           coalesced along c (one contiguous run with one member) and every later read is of LDS; a wider slab is read from
//           memory by the rows phase, coalesced along c, and a second time by the columns phase (from L2).
//   rows    a team of L = min(64, the least power of two >= C) adjacent lanes per row, R = 256 / L rows at a time, lane l the
//           columns c = l (mod L) ascending.
//           GP = 1 for C > 64, else the largest power of two <= max(1, R / N): small slabs share a workgroup.
//   columns C <= 64: thread (group of the pack, part k, column c), RS = min(16, R / GP) contiguous parts
//           [k N / RS, (k + 1) N / RS) of the rows; C > 64: thread t the columns c = t (mod 256) ascending, all rows.
//   paths   TN = min(64, 256 / GP) adjacent lanes per group, lane i the paths n = i (mod TN) ascending.
// Summation order (a function of N and C alone; L, R, GP, RS and TN follow from them):
//   row n: lane l the online pair (m, s): for a logit z above the running maximum m, s = s expf(m - z) + 1 and m = z, otherwise
//   s += expf(z - m) (one expf per logit; the shift is 0 while m = -Inf); the row's maximum m' by a butterfly over the L lanes,
//   each lane's s scaled once, s expf(m - m'), and the L products added by a butterfly (xor 1, .., L / 2); then ls = logf(s) and
//   lp_c = (z_c - m') - ls, so a common shift of a row's logits cancels before anything rounds against it.  logp = lp_y, the
//   label's logit and class weight picked out by comparing the column index with the label (the label forms no address).
//   binary: m = max(0, z), s = expf(0 - m) + expf(z - m).
//   probs_c: p_nc = expf(lp_nc) added n ascending inside each part, the parts k ascending, divided by N.  The same thread adds
//   its p lp (p = 0: +0) in the order it meets them (C > 64: columns outer, rows inner), then parts k ascending; entropy adds
//   -pbar logf(pbar) (pbar = 0: +0), C > 64: per thread c ascending.  Both sums then go over the min(CP, 64) column lanes by a
//   butterfly (xor 1, ..) and, for C > 64, over the four waves in order.  binary: pbar_0 is summed like pbar_1, not 1 - pbar_1.
//   nll, xent: a_n = logp_n + logw_n; max over n; lane i the chains sum += expf(a_n - max) and sum += logp_n over n = i (mod TN)
//   ascending, the lanes by a butterfly; nll = -w (max + logf(sum) - logf(N)), xent = -w (sum / N).  A NaN a_n gives NaN, an
//   infinite maximum max - logf(N).
// Backward: the staging and the rows phase again, then per group r_n = softmax_n(a_n) in the paths layout (expf(a_n - max) /
// sum) and k_n = w (grad_nll r_n + grad_xent / N) - grad_logp_n in LDS, then the teams walk their rows once more:
// grad_logits = k_n (expf(lp_nc) - [c == y]).  No atomics, no workspace, nothing depends on the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "snsde.h"
#include "snsde_internal.h"
#include "snsde_sample_set.h"      // MAX_N, pooled_row, pooled_dims_ok

namespace {

constexpr int TH = 256;             // threads of a workgroup
constexpr int SLAB_MAX = 24576;     // floats of a pack's slab staged in LDS
constexpr int RS_MAX = 16;          // row parts of the column sums
constexpr int FIXED = 7 * TH + 8;   // floats of LDS in front of the slab: m, ls, a, w, and the part sums p, q, e; 8 wave sums

struct CDims {
    int64_t OG, G, ostride, mstride, packs;      // OG = outer G groups; ostride = M G S C, mstride = G S C; packs = ceil(OG / GP)
    int32_t S, C, N, L, lshift, R, GP, CP, cpshift, RS, rsshift, TN, tnshift, staged;
};

__device__ __forceinline__ int64_t group_base(int64_t gi, const CDims& d) {
    const int64_t o = gi / d.G, g = gi - o * d.G;
    return o * d.ostride + g * d.S * (int64_t)d.C;
}

__device__ __forceinline__ int64_t row_of(int n, const CDims& d) {
    if (d.S == d.N) return (int64_t)n * d.C;      // (uniform: one member)
    return pooled_row(n, d.S, d.C, d.mstride);
}

__device__ __forceinline__ float team_sum(float x, int lanes) {
    for (int k = 1; k < lanes; k <<= 1) x += __shfl_xor(x, k, 64);      // (uniform trip count; the lanes are adjacent)
    return x;
}

__device__ __forceinline__ float plogp(float p, float lp) { return p == 0.0f ? 0.0f : p * lp; }
__device__ __forceinline__ float neg_plogp(float p) { return p == 0.0f ? 0.0f : -p * logf(p); }

struct Lds {
    float *m, *ls, *a, *w, *p, *q, *e, *red, *slab;
};

__device__ __forceinline__ Lds carve(float* lds) {
    Lds s;
    s.m = lds; s.ls = lds + TH; s.a = lds + 2 * TH; s.w = lds + 3 * TH; s.p = lds + 4 * TH; s.q = lds + 5 * TH; s.e = lds + 6 * TH;
    s.red = lds + 7 * TH; s.slab = lds + FIXED;
    return s;
}

// The pack's slab from memory into LDS, all 256 threads, element i = (row r of the pack, column c) to slab[i]: with one member
// the rows of adjacent groups follow each other in memory and the copy is one contiguous run.
__device__ __forceinline__ void stage_slab(const float* __restrict__ logits, const CDims& d, int64_t g0, float* __restrict__ slab) {
    const int64_t left = d.OG - g0;
    const int total = (int)(left < d.GP ? left : d.GP) * d.N * d.C;
    if (d.S == d.N) {      // (uniform: one member - group gi starts at gi N C, whatever its outer slice)
        const float* src = logits + group_base(g0, d);
#pragma unroll 8
        for (int i = threadIdx.x; i < total; i += TH) slab[i] = src[i];
    } else {
        const int per = d.N * d.C;
#pragma unroll 4
        for (int i = threadIdx.x; i < total; i += TH) {
            const int gp = i / per, j = i - gp * per;
            const int n = j / d.C, c = j - n * d.C;
            slab[i] = logits[group_base(g0 + gp, d) + row_of(n, d) + c];
        }
    }
}

// The rows phase of a pack: m (the maximum, 0 for -Inf), ls = log sum exp(z - m), a = logp of every row, w of every group.
// The rows come from the staged slab where there is one, else from memory.
template <bool BIN>
__device__ __forceinline__ void rows_phase(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                           const float* __restrict__ cw, const CDims& d, int64_t g0, const Lds& s) {
    const int tid = threadIdx.x, tm = tid >> d.lshift, l = tid & (d.L - 1);
    const int rows = d.GP * d.N;
    const int y0 = labels ? labels[g0] : -1;      // (the label of a pack of one group, fetched once)
    for (int r0 = 0; r0 < rows; r0 += d.R) {      // (uniform trip count: the butterflies below run in every lane)
        const int r = r0 + tm;
        const int gp = r / d.N, n = r - gp * d.N;
        const int64_t gi = g0 + gp;
        const bool live = r < rows && gi < d.OG;
        float m = -INFINITY, sum = 0.0f, zy = 0.0f, wy = 0.0f, z1 = 0.0f;
        int y = -1;
        if (live) {
            y = d.GP == 1 || !labels ? y0 : labels[gi];
            const float* row = d.staged ? s.slab + (size_t)r * d.C : logits + group_base(gi, d) + row_of(n, d);
            if (BIN) {
                z1 = row[0];
                m = fmaxf(0.0f, z1);
                sum = __fadd_rn(expf(0.0f - m), expf(z1 - m));
                zy = y == 1 ? z1 : 0.0f;
                wy = !cw ? 1.0f : y == 1 ? cw[1] : cw[0];
            } else {
                for (int c = l; c < d.C; c += d.L) {
                    const float z = row[c];
                    const bool up = z > m;
                    const float e = expf(up ? m - z : z - (m == -INFINITY ? 0.0f : m));
                    sum = up ? __fadd_rn(__fmul_rn(sum, e), 1.0f) : __fadd_rn(sum, e);
                    m = up ? z : m;
                    if (c == y) {      // (the label selects; the address is the column's)
                        zy = z;
                        wy = cw ? cw[c] : 1.0f;
                    }
                }
            }
        }
        if (!BIN) {
            float mt = m;
            for (int k = 1; k < d.L; k <<= 1) mt = fmaxf(mt, __shfl_xor(mt, k, 64));
            sum = __fmul_rn(sum, expf(m - (mt == -INFINITY ? 0.0f : mt)));      // (the lane's own maximum: a factor of exactly 1)
            m = mt;
            for (int k = 1; k < d.L; k <<= 1) {
                sum += __shfl_xor(sum, k, 64);
                zy += __shfl_xor(zy, k, 64);      // (one lane holds the value, the others +0)
                wy += __shfl_xor(wy, k, 64);
            }
        }
        if (live && l == 0) {
            const float msh = m == -INFINITY ? 0.0f : m, ls = logf(sum);
            const int classes = BIN ? 2 : d.C;
            s.m[r] = msh;
            s.ls[r] = ls;
            s.a[r] = y < 0 ? 0.0f : y >= classes ? NAN : (zy - msh) - ls;
            if (n == 0) s.w[gp] = wy;
        }
    }
}

// max, sum of expf(a_n - max) and sum of logp_n over the paths of a group, lane i of TN; bad: a NaN among the a_n
__device__ __forceinline__ void paths_sums(const float* __restrict__ logw, const CDims& d, int64_t gi, int gp, int i, const Lds& s,
                                           float& mx, float& sum, float& xs, bool& bad) {
    mx = -INFINITY; sum = 0.0f; xs = 0.0f;
    float nan = 0.0f;
    for (int n = i; n < d.N; n += d.TN) {
        const float a = logw ? s.a[gp * d.N + n] + logw[gi * d.N + n] : s.a[gp * d.N + n];
        nan = a != a ? 1.0f : nan;
        mx = fmaxf(mx, a);
    }
    for (int k = 1; k < d.TN; k <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, k, 64));
        nan = fmaxf(nan, __shfl_xor(nan, k, 64));
    }
    bad = nan != 0.0f;
    for (int n = i; n < d.N; n += d.TN) {
        const float lp = s.a[gp * d.N + n];
        const float a = logw ? lp + logw[gi * d.N + n] : lp;
        sum += expf(a - mx);
        xs += lp;
    }
    sum = team_sum(sum, d.TN);
    xs = team_sum(xs, d.TN);
}

template <bool BIN>
__global__ void __launch_bounds__(TH) snsde_sample_class_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                                const float* __restrict__ logw, const float* __restrict__ cw, CDims d,
                                                                float* __restrict__ logp, float* __restrict__ nll,
                                                                float* __restrict__ xent, float* __restrict__ probs,
                                                                float* __restrict__ entropy, float* __restrict__ expent) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds s = carve(lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float fN = (float)d.N;
    // the columns phase: thread = (q = group of the pack and part, column lane cl)
    const int cl = tid & (d.CP - 1), q = tid >> d.cpshift;
    const int cgp = q >> d.rsshift, ck = q & (d.RS - 1);
    const int n0 = ck * d.N / d.RS, n1 = (ck + 1) * d.N / d.RS;
    // the paths phase: thread = (group of the pack, lane pi of TN)
    const int pgp = tid >> d.tnshift, pi = tid & (d.TN - 1);
    for (int64_t pack = blockIdx.x; pack < d.packs; pack += gridDim.x) {
        const int64_t g0 = pack * d.GP;
        __syncthreads();      // (the last pack has been read)
        if (d.staged) {      // (uniform)
            stage_slab(logits, d, g0, s.slab);
            __syncthreads();
        }
        rows_phase<BIN>(logits, labels, cw, d, g0, s);
        __syncthreads();
        // columns: probs, entropy, expected entropy
        {
            const int64_t gi = g0 + cgp;
            const bool live = cgp < d.GP && gi < d.OG;
            const int64_t base = live ? group_base(gi, d) : 0;
            float ps = 0.0f, ps0 = 0.0f, es = 0.0f, hs = 0.0f;
            if (live) {
                if (BIN) {
                    for (int n = n0; n < n1; ++n) {
                        const int r = cgp * d.N + n;
                        const float z = d.staged ? s.slab[r] : logits[base + row_of(n, d)];
                        const float m = s.m[r], ls = s.ls[r];
                        const float lp0 = (0.0f - m) - ls, lp1 = (z - m) - ls;
                        const float p0 = expf(lp0), p1 = expf(lp1);
                        ps0 += p0;
                        ps += p1;
                        es += plogp(p0, lp0);
                        es += plogp(p1, lp1);
                    }
                } else {
                    for (int c = cl; c < d.C; c += d.CP) {
                        ps = 0.0f;
#pragma unroll 4
                        for (int n = n0; n < n1; ++n) {
                            const int r = cgp * d.N + n;
                            const float z = d.staged ? s.slab[(size_t)r * d.C + c] : logits[base + row_of(n, d) + c];
                            const float lp = (z - s.m[r]) - s.ls[r];
                            const float p = expf(lp);
                            ps += p;
                            es += plogp(p, lp);
                        }
                        if (d.RS == 1) {
                            const float pb = ps / fN;
                            probs[gi * d.C + c] = pb;
                            hs += neg_plogp(pb);
                        }
                    }
                }
            }
            if (d.RS > 1 || BIN) {      // (uniform) the parts in order, by the thread of part 0
                s.p[tid] = ps;
                s.q[tid] = ps0;
                s.e[tid] = es;
                __syncthreads();
                hs = es = 0.0f;
                if (live && ck == 0 && cl < d.C) {
                    for (int k = 1; k < d.RS; ++k) ps += s.p[tid + (k << d.cpshift)];
                    for (int k = 0; k < d.RS; ++k) es += s.e[tid + (k << d.cpshift)];
                    const float pb = ps / fN;
                    probs[gi * d.C + cl] = pb;
                    hs = neg_plogp(pb);
                    if (BIN) {
                        for (int k = 1; k < d.RS; ++k) ps0 += s.q[tid + (k << d.cpshift)];
                        hs += neg_plogp(ps0 / fN);
                    }
                }
            }
            hs = team_sum(hs, d.CP < 64 ? d.CP : 64);
            es = team_sum(es, d.CP < 64 ? d.CP : 64);
            if (d.CP > 64) {      // (uniform: C > 64, one group, all four waves)
                if (lane == 0) {
                    s.red[wave] = hs;
                    s.red[4 + wave] = es;
                }
                __syncthreads();
                hs = ((s.red[0] + s.red[1]) + s.red[2]) + s.red[3];
                es = ((s.red[4] + s.red[5]) + s.red[6]) + s.red[7];
            }
            if (live && ck == 0 && cl == 0) {
                entropy[gi] = hs;
                expent[gi] = -es / fN;
            }
        }
        // paths: logp, nll, xent
        {
            const int64_t gi = g0 + pgp;
            if (pgp < d.GP && gi < d.OG) {      // (whole teams of TN adjacent lanes)
                float mx, sum, xs;
                bool bad;
                paths_sums(logw, d, gi, pgp, pi, s, mx, sum, xs, bad);
                for (int n = pi; n < d.N; n += d.TN) logp[gi * d.N + n] = s.a[pgp * d.N + n];
                if (pi == 0) {
                    const int y = labels ? labels[gi] : -1;
                    const float w = s.w[pgp];
                    const float lse = bad ? NAN : isinf(mx) ? mx : mx + logf(sum);
                    nll[gi] = y < 0 ? 0.0f : -w * (lse - logf(fN));
                    xent[gi] = y < 0 ? 0.0f : -w * (xs / fN);
                }
            }
        }
    }
}

template <bool BIN>
__global__ void __launch_bounds__(TH) snsde_sample_class_backward_kernel(const float* __restrict__ gnll, const float* __restrict__ gxent,
                                                                         const float* __restrict__ glogp, const float* __restrict__ logits,
                                                                         const int32_t* __restrict__ labels, const float* __restrict__ logw,
                                                                         const float* __restrict__ cw, CDims d, float* __restrict__ glogits,
                                                                         float* __restrict__ glogw) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Lds s = carve(lds);
    float* kbuf = s.p;
    const int tid = threadIdx.x;
    const float fN = (float)d.N;
    const int pgp = tid >> d.tnshift, pi = tid & (d.TN - 1);
    const int tm = tid >> d.lshift, l = tid & (d.L - 1);
    const int rows = d.GP * d.N, classes = BIN ? 2 : d.C;
    for (int64_t pack = blockIdx.x; pack < d.packs; pack += gridDim.x) {
        const int64_t g0 = pack * d.GP;
        __syncthreads();      // (the last pack has been read)
        if (d.staged) {      // (uniform)
            stage_slab(logits, d, g0, s.slab);
            __syncthreads();
        }
        rows_phase<BIN>(logits, labels, cw, d, g0, s);
        __syncthreads();
        {
            const int64_t gi = g0 + pgp;
            if (pgp < d.GP && gi < d.OG) {
                const int y = labels ? labels[gi] : -1;
                const float w = s.w[pgp];
                const float gn = gnll ? gnll[gi] : 0.0f, gx = gxent ? gxent[gi] / fN : 0.0f;
                float mx = 0.0f, sum = 1.0f, xs;
                bool bad = false;
                if (gnll) paths_sums(logw, d, gi, pgp, pi, s, mx, sum, xs, bad);      // (uniform: the softmax is needed only by grad_nll)
                for (int n = pi; n < d.N; n += d.TN) {
                    const int64_t at = gi * d.N + n;
                    float rn = 0.0f;
                    if (gnll) {
                        const float lp = s.a[pgp * d.N + n];
                        rn = bad ? NAN : expf((logw ? lp + logw[at] : lp) - mx) / sum;
                    }
                    const float wr = w * (gn * rn);
                    const float k = (wr + w * gx) - (glogp ? glogp[at] : 0.0f);
                    kbuf[pgp * d.N + n] = y < 0 ? 0.0f : y >= classes ? NAN : k;
                    if (glogw) glogw[at] = y < 0 ? 0.0f : -wr;
                }
            }
        }
        __syncthreads();
        const int y0 = labels ? labels[g0] : -1;
        for (int r = tm; r < rows; r += d.R) {
            const int gp = r / d.N, n = r - gp * d.N;
            const int64_t gi = g0 + gp;
            if (gi >= d.OG) break;
            const int y = d.GP == 1 || !labels ? y0 : labels[gi];
            const int64_t at = group_base(gi, d) + row_of(n, d);
            const float m = s.m[r], ls = s.ls[r], k = kbuf[r];
            const float* row = d.staged ? s.slab + (size_t)r * d.C : logits + at;
            if (BIN) {
                const float p1 = expf((row[0] - m) - ls);
                glogits[at] = y < 0 ? 0.0f : k * (p1 - (y == 1 ? 1.0f : 0.0f));
            } else {
                for (int c = l; c < d.C; c += d.L) {
                    const float p = expf((row[c] - m) - ls);
                    glogits[at + c] = y < 0 ? 0.0f : k * (p - (c == y ? 1.0f : 0.0f));
                }
            }
        }
    }
}

int shift_of(int p) {
    int s = 0;
    while ((1 << s) < p) ++s;
    return s;
}

// (outer, M, G, S, C): positive, the element count fits 63 bits, N = M S within the cap, binary only at width 1
bool class_dims(int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t binary, CDims* d) {
    int64_t per;
    if (!pooled_dims_ok(outer, members, groups, samples, width, &per) || (binary && width != 1)) return false;
    d->G = groups; d->OG = outer * groups; d->mstride = per; d->ostride = members * per;
    d->S = samples; d->C = width; d->N = members * samples;
    int L = 1;
    while (L < 64 && L < width) L *= 2;
    d->L = L; d->lshift = shift_of(L); d->R = TH / L;
    int GP = 1;
    if (width <= 64) while (2 * GP * d->N <= d->R) GP *= 2;
    d->GP = GP;
    d->CP = width <= 64 ? L : TH; d->cpshift = shift_of(d->CP);
    d->RS = width <= 64 ? (d->R / GP < RS_MAX ? d->R / GP : RS_MAX) : 1; d->rsshift = shift_of(d->RS);
    d->TN = TH / GP < 64 ? TH / GP : 64; d->tnshift = shift_of(d->TN);
    d->staged = (int64_t)GP * d->N * width <= SLAB_MAX;
    d->packs = (d->OG + GP - 1) / GP;
    return true;
}

}  // namespace

extern "C" int snsde_sample_class(const float* logits, const int32_t* labels, const float* logw, const float* class_weight,
                                  int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t binary,
                                  float* logp, float* nll, float* xent, float* probs, float* entropy, float* expent, void* hip_stream) {
    if (!logits || !logp || !nll || !xent || !probs || !entropy || !expent) return SNSDE_ERR_NULL;
    CDims d;
    if (!class_dims(outer, members, groups, samples, width, binary, &d)) return SNSDE_ERR_DIMS;
    static SnsdeLdsAttr seen[2];
    const size_t lds = (FIXED + (d.staged ? (size_t)d.GP * d.N * d.C : 0)) * sizeof(float);
    auto kernel = binary ? snsde_sample_class_kernel<true> : snsde_sample_class_kernel<false>;
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(kernel), lds, seen[binary ? 1 : 0]);
    if (rc != SNSDE_OK) return rc;
    const unsigned grid = (unsigned)(d.packs < 4096 ? d.packs : 4096);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), lds, static_cast<hipStream_t>(hip_stream), logits, labels, logw, class_weight, d,
                       logp, nll, xent, probs, entropy, expent);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

extern "C" int snsde_sample_class_backward(const float* grad_nll, const float* grad_xent, const float* grad_logp, const float* logits,
                                           const int32_t* labels, const float* logw, const float* class_weight, int64_t outer,
                                           int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t binary,
                                           float* grad_logits, float* grad_logw, void* hip_stream) {
    if (!logits || !grad_logits) return SNSDE_ERR_NULL;
    CDims d;
    if (!class_dims(outer, members, groups, samples, width, binary, &d)) return SNSDE_ERR_DIMS;
    static SnsdeLdsAttr seen[2];
    const size_t lds = (FIXED + (d.staged ? (size_t)d.GP * d.N * d.C : 0)) * sizeof(float);
    auto kernel = binary ? snsde_sample_class_backward_kernel<true> : snsde_sample_class_backward_kernel<false>;
    const int rc = snsde_lds_attr(reinterpret_cast<const void*>(kernel), lds, seen[binary ? 1 : 0]);
    if (rc != SNSDE_OK) return rc;
    const unsigned grid = (unsigned)(d.packs < 4096 ? d.packs : 4096);      // (the kernel strides over the rest)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TH), lds, static_cast<hipStream_t>(hip_stream), grad_nll, grad_xent, grad_logp, logits,
                       labels, logw, class_weight, d, grad_logits, grad_logw);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
