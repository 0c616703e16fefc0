// Gradient of the fused solve with respect to the control path (include/snsde.h: snsde_coeff_gradients), gfx950.
//
// X(t) enters the drift's first layer only, and linearly: with delta_p (B, H) = dL/d(pre-activation of the first rectified layer)
// at drift pass p (delta_save slot snsde_save::delta_first, the one the weight-gradient pass reads for the folded first layer) and
//     M (H, C) = emb.weight[:, H:] . initial_network.weight   (input_option 2 / 4 / 6),   initial_network.weight   (input_option 0)
// the cotangent of X(t_p) is v_p = delta_p . M (B, C), and the spline a + (b + (two_c / 2 + three_d r / 3) r) r spreads it over
// the four coefficient blocks of the pass's interval k_p with the weights phi(r_p) = (1, r, r^2 / 2, r^3 / 3):
//     grad_coeffs[b, k, j C + c] = sum_{p : k_p = k} phi_j(r_p) v_p[b, c].
// (k_p, r_p): step_tab columns 5 / 4; SRK: the stage-table slot of the pass's drift stage - passes 3n + {0, 1, 2} are the drift
// evaluations at t0, t0 + h, t0 + h / 2 = slots 0, 3, 2, the order snsde_srk_expand_kernel gives the forward.
//
// Three launches and a memset on the caller's stream, no atomics:
//   1. snsde_cgrad_fold_kernel   M into the workspace (H C floats; a copy for input_option 0);
//   2. snsde_cgrad_vjp_kernel    v = delta . M for every (pass, row): tiles of 32 reduction rows staged in LDS with 16-byte loads
//                                (adjacent lanes on adjacent h), M in LDS, every output one fmaf chain over ascending h;
//   3. snsde_cgrad_walk_kernel   one lane per (row, channel) walks the passes in ascending order with the four sums of the current
//                                interval in registers; when the interval changes it stores them and loads the new interval's (zero
//                                from the memset, or - SRK, whose stage times are not monotone in pass order - what the same lane
//                                stored before: a store and a reload do not change the value, so every (b, k, j, c) is one
//                                owner's sum in ascending pass order).
// A row's result depends on that row's delta planes and the tables only: bit-equal run to run and under any batch sharding.
// Sample paths (snsde_solve::samples = S > 1 under SNSDE_FLAG_SAMPLE_GRAD): delta and v stay per path (B = paths), grad_coeffs is
// per input row (B / S rows) and snsde_cgrad_walk_groups_kernel takes launch 3: it sums over the S paths of a row where it walks
// the passes - passes ascending and, inside a pass, the row's paths s = 0 .. S-1: one owner per element, one fmaf chain.  A path
// with zero planes adds exact zeros, so with the cotangent on one path of a group the sums are those of that path's own walk, bit
// for bit.  The S values of (pass, input row) are S C adjacent floats of v: a workgroup owns RB input rows, ALL its lanes fetch the
// rows' RB S C contiguous floats of up to eight passes into LDS (coalesced, eight loads in flight per lane: the memory
// parallelism of the one-path walk), then the first RB C lanes run the chains out of LDS.  Where one pass of one row does not fit
// the LDS (S C > 16320 floats) the round holds one pass and a chunk of its paths, in the same order.
// The intermediate v costs P B C floats of traffic twice beside the P B H floats of delta (a third more at the K2 shape); in
// exchange both kernels are fully parallel instead of one workgroup per row tile walking its passes one after the other.
#include "snsde_internal.h"

namespace {

constexpr int TR = 32;             // reduction rows ((pass, batch row) pairs) per tile
constexpr int NT = 256;
constexpr int LDS_FLOATS = 16384 - 64;      // 64 KiB of LDS, the size every kernel may use without an attribute

struct CArgs {
    const float* delta;            // (P, NG, B, H)
    const float* params;
    const float* step_tab;         // (N, SNSDE_STEP_STRIDE)
    const float* srk_tab;          // (N, 4, SNSDE_SRK_STRIDE), SRK
    float* M;                      // (H, C)
    float* v;                      // (P B, C)
    float* grad;                   // (B, L - 1, 4 C)
    int64_t R;                     // P B
    int32_t B, H, C, Lm1, P, NG, slot, srk, CC, LDH;
    int32_t S;                     // paths per input row (>= 1): v and delta have B rows per pass, grad B / S rows
    int32_t RB, SEG, WBS, SCH;     // walk_groups: input rows per workgroup, floats of a pass in an LDS round (RB SCH C), passes per
                                   // round (<= 8), paths per round (S; fewer - then RB = WBS = 1 - where S C floats exceed the LDS)
    int32_t emb_w, init_w, fold;   // float offsets of emb.weight / initial_network.weight in params
};

__global__ __launch_bounds__(256) void snsde_cgrad_fold_kernel(CArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.H * a.C) return;
    const int h = i / a.C, c = i - h * a.C;
    const float* W = a.params + a.init_w;                       // (H, C)
    if (!a.fold) { a.M[i] = W[i]; return; }
    const float* E = a.params + a.emb_w + (size_t)h * 2 * a.H + a.H;      // emb.weight[h, H:]
    float s = 0.0f;
    for (int j = 0; j < a.H; ++j) s = fmaf(E[j], W[(size_t)j * a.C + c], s);
    a.M[i] = s;
}

// blockIdx.y = channel chunk [c0, c0 + CC); blockIdx.x strides over the row tiles
__global__ __launch_bounds__(NT) void snsde_cgrad_vjp_kernel(CArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int H = a.H, LDH = a.LDH;
    const int c0 = blockIdx.y * a.CC;
    const int cc = a.C - c0 < a.CC ? a.C - c0 : a.CC;
    float* Ms = lds;                       // (H, cc)
    float* Ds = lds + (size_t)H * a.CC;    // (TR, LDH)
    for (int i = threadIdx.x; i < H * cc; i += NT) {
        const int h = i / cc, c = i - h * cc;
        Ms[i] = a.M[(size_t)h * a.C + c0 + c];
    }
    const int64_t ntiles = (a.R + TR - 1) / TR;
    const int H4 = H / 4;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();                   // (the previous tile's readers; the first pass: Ms)
        for (int i = threadIdx.x; i < TR * H4; i += NT) {
            const int r = i / H4, h4 = i - r * H4;
            const int64_t q = tile * TR + r;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < a.R) {
                const int64_t p = q / a.B, b = q - p * a.B;
                d = *reinterpret_cast<const float4*>(a.delta + (((size_t)p * a.NG + a.slot) * a.B + b) * H + 4 * h4);
            }
            *reinterpret_cast<float4*>(Ds + r * LDH + 4 * h4) = d;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < (TR / 4) * cc; i += NT) {
            const int rg = i / cc, c = i - rg * cc;
            const float* d0 = Ds + (rg * 4) * LDH;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int h = 0; h < H; h += 4) {
                const float m0 = Ms[h * cc + c], m1 = Ms[(h + 1) * cc + c], m2 = Ms[(h + 2) * cc + c], m3 = Ms[(h + 3) * cc + c];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float4 d = *reinterpret_cast<const float4*>(d0 + rr * LDH + h);
                    acc[rr] = fmaf(d.w, m3, fmaf(d.z, m2, fmaf(d.y, m1, fmaf(d.x, m0, acc[rr]))));
                }
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int64_t q = tile * TR + rg * 4 + rr;
                if (q < a.R) a.v[(size_t)q * a.C + c0 + c] = acc[rr];
            }
        }
    }
}

__device__ __forceinline__ void pass_interval(const CArgs& a, int p, float* frac, int* idx) {
    int k;
    if (a.srk) {
        const int n = p / 3, stg = p - 3 * n;
        const float* row = a.srk_tab + ((size_t)n * 4 + (stg == 0 ? 0 : (stg == 1 ? 3 : 2))) * SNSDE_SRK_STRIDE;
        *frac = row[3]; k = __float_as_int(row[4]);
    } else {
        const float* row = a.step_tab + (size_t)p * SNSDE_STEP_STRIDE;
        *frac = row[4]; k = __float_as_int(row[5]);
    }
    k = k < 0 ? 0 : k;
    *idx = k > a.Lm1 - 1 ? a.Lm1 - 1 : k;
}

constexpr int WB = 8;      // passes whose v loads are in flight together

__global__ __launch_bounds__(64) void snsde_cgrad_walk_kernel(CArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t BC = (int64_t)a.B * a.C;
    if (i >= BC) return;
    const int64_t b = i / a.C;
    const int c = (int)(i - b * a.C);
    const int C = a.C;
    const float* v = a.v + i;
    float* out = a.grad + (size_t)b * a.Lm1 * 4 * C + c;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int cur = -1;
    for (int p0 = 0; p0 < a.P; p0 += WB) {
        float vv[WB];
#pragma unroll
        for (int j = 0; j < WB; ++j) vv[j] = p0 + j < a.P ? v[(size_t)(p0 + j) * BC] : 0.0f;
#pragma unroll
        for (int j = 0; j < WB; ++j) {
            if (p0 + j >= a.P) break;
            float r; int k;
            pass_interval(a, p0 + j, &r, &k);
            if (k != cur) {
                if (cur >= 0) {
                    float* o = out + (size_t)cur * 4 * C;
                    o[0] = s0; o[C] = s1; o[2 * C] = s2; o[3 * C] = s3;
                }
                cur = k;
                const float* o = out + (size_t)cur * 4 * C;
                s0 = o[0]; s1 = o[C]; s2 = o[2 * C]; s3 = o[3 * C];
            }
            const float x = vv[j];
            s0 += x;
            s1 = fmaf(r, x, s1);
            s2 = fmaf(0.5f * r * r, x, s2);
            s3 = fmaf(r * r * r / 3.0f, x, s3);
        }
    }
    if (cur >= 0) {
        float* o = out + (size_t)cur * 4 * C;
        o[0] = s0; o[C] = s1; o[2 * C] = s2; o[3 * C] = s3;
    }
}

constexpr int WNT = 256;      // threads of a walk_groups workgroup
constexpr int WBMAX = 8;      // passes per LDS round

__global__ __launch_bounds__(WNT) void snsde_cgrad_walk_groups_kernel(CArgs a) {
    extern __shared__ __align__(16) float lds[];        // (WBS, SEG)
    const int C = a.C, S = a.S, SEG = a.SEG, wb = a.WBS, SCH = a.SCH;
    const int64_t rows = a.B / S;
    const int64_t b0 = (int64_t)blockIdx.x * a.RB;
    const int rbn = rows - b0 < a.RB ? (int)(rows - b0) : a.RB;      // input rows of this workgroup (>= 1 by the grid)
    const int64_t BC = (int64_t)a.B * C;
    const float* v = a.v + (size_t)b0 * S * C;
    const bool owner = (int)threadIdx.x < rbn * C;
    const int rb = owner ? (int)threadIdx.x / C : 0, c = owner ? (int)threadIdx.x - rb * C : 0;
    float* out = a.grad + (size_t)(b0 + rb) * a.Lm1 * 4 * C + c;
    const float* mine = lds + rb * S * C + c;          // (a chunked round has RB = 1: rb = 0)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int cur = -1;
    for (int p0 = 0; p0 < a.P; p0 += wb) {
        const int np = a.P - p0 < wb ? a.P - p0 : wb;
        for (int sb = 0; sb < S; sb += SCH) {          // one trip (SCH = S) unless S C floats exceed the LDS: paths sb .. sb + sc - 1
            const int sc = S - sb < SCH ? S - sb : SCH;
            const int seg = SCH == S ? rbn * S * C : sc * C;      // the round's floats of one pass of v: contiguous
            const float* vs = v + (size_t)sb * C;
            __syncthreads();                   // (the previous round's readers)
            for (int i = threadIdx.x; i < seg; i += WNT) {
                float t[WBMAX];
#pragma unroll
                for (int j = 0; j < WBMAX; ++j) t[j] = j < np ? vs[(size_t)(p0 + j) * BC + i] : 0.0f;
#pragma unroll
                for (int j = 0; j < WBMAX; ++j) if (j < np) lds[j * SEG + i] = t[j];
            }
            __syncthreads();
            if (owner) {
                for (int j = 0; j < np; ++j) {
                    float r; int k;
                    pass_interval(a, p0 + j, &r, &k);
                    if (k != cur) {            // (a later chunk of the same pass: k == cur)
                        if (cur >= 0) {
                            float* o = out + (size_t)cur * 4 * C;
                            o[0] = s0; o[C] = s1; o[2 * C] = s2; o[3 * C] = s3;
                        }
                        cur = k;
                        const float* o = out + (size_t)cur * 4 * C;
                        s0 = o[0]; s1 = o[C]; s2 = o[2 * C]; s3 = o[3 * C];
                    }
                    const float f2 = 0.5f * r * r, f3 = r * r * r / 3.0f;
                    const float* x_ = mine + j * SEG;
                    for (int s = 0; s < sc; ++s) {
                        const float x = x_[s * C];
                        s0 += x;
                        s1 = fmaf(r, x, s1);
                        s2 = fmaf(f2, x, s2);
                        s3 = fmaf(f3, x, s3);
                    }
                }
            }
        }
    }
    if (owner && cur >= 0) {
        float* o = out + (size_t)cur * 4 * C;
        o[0] = s0; o[C] = s1; o[2 * C] = s2; o[3 * C] = s3;
    }
}

// channels per chunk of the vjp kernel so that M's chunk and one row tile share 64 KiB of LDS (0: H too large)
int chunk_channels(int H, int C) {
    const int room = LDS_FLOATS - TR * (H + 4);
    if (room < H) return 0;
    const int cc = room / H;
    return cc < C ? cc : C;
}

size_t m_floats(const snsde_solve& s) {
    return ((size_t)s.model.hidden_channels * s.model.input_channels + 63) & ~(size_t)63;
}

}  // namespace

bool snsde_cgrad_reads_x(const snsde_model& m) { return m.input_option == 0 || m.input_option == 2 || m.input_option == 4 || m.input_option == 6; }

size_t snsde_cgrad_workspace_floats(const snsde_solve& s) {
    if (!snsde_cgrad_reads_x(s.model)) return 0;
    const size_t P = (size_t)s.n_steps * (s.method == SNSDE_SRK ? 3 : 1);
    return m_floats(s) + P * s.batch * s.model.input_channels + 64;
}

int snsde_cgrad_zero_launch(const snsde_solve& s, float* grad_coeffs, hipStream_t stream) {
    const size_t bytes = (size_t)(s.batch / snsde_samples(&s)) * (s.knots - 1) * 4 * s.model.input_channels * sizeof(float);      // (input rows)
    return hipMemsetAsync(grad_coeffs, 0, bytes, stream) == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

int snsde_cgrad_launch(const snsde_backward* b, const SnsdeNet& net, int delta_slots, float* grad_coeffs, float* ws, hipStream_t stream) {
    const snsde_solve& s = b->fwd;
    const int H = s.model.hidden_channels, C = s.model.input_channels, io = s.model.input_option;
    const bool emb = io == 2 || io == 4 || io == 6;
    const int nhid = s.model.num_hidden_layers - 1;
    if (!snsde_cgrad_reads_x(s.model) || !net.init.present || (emb && !net.emb.present)) return SNSDE_ERR_UNSUPPORTED;
    if (H % 4 != 0 || snsde_save::delta_first(nhid) >= delta_slots) return SNSDE_ERR_UNSUPPORTED;
    const int CC = chunk_channels(H, C);
    if (CC < 1) return SNSDE_ERR_LDS;
    CArgs a{};
    a.delta = b->delta_save; a.params = s.params; a.step_tab = s.step_tab; a.srk_tab = s.srk_tab;
    a.M = ws; a.v = ws + m_floats(s); a.grad = grad_coeffs;
    a.srk = s.method == SNSDE_SRK ? 1 : 0;
    a.P = s.n_steps * (a.srk ? 3 : 1);
    a.B = s.batch; a.H = H; a.C = C; a.Lm1 = s.knots - 1; a.NG = delta_slots; a.slot = snsde_save::delta_first(nhid);
    a.S = snsde_samples(&s);
    if (a.B % a.S != 0) return SNSDE_ERR_DIMS;
    if (a.S > 1 && C > WNT) return SNSDE_ERR_UNSUPPORTED;      // (walk_groups: a lane per channel of a row; the MFMA paths stop at C = 80)
    a.R = (int64_t)a.P * a.B;
    a.CC = CC; a.LDH = H + 4;
    a.emb_w = emb ? net.emb.src_w : 0; a.init_w = net.init.src_w; a.fold = emb ? 1 : 0;
    int rc = snsde_cgrad_zero_launch(s, grad_coeffs, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(snsde_cgrad_fold_kernel, dim3((H * C + 255) / 256), dim3(256), 0, stream, a);
    const int64_t ntiles = (a.R + TR - 1) / TR;
    const int gx = (int)(ntiles < 1024 ? ntiles : 1024);
    const size_t lds_bytes = ((size_t)H * CC + (size_t)TR * a.LDH) * sizeof(float);
    hipLaunchKernelGGL(snsde_cgrad_vjp_kernel, dim3(gx, (C + CC - 1) / CC), dim3(NT), lds_bytes, stream, a);
    const int64_t BC = (int64_t)(a.B / a.S) * C;      // one lane per (input row, channel)
    if (a.S > 1) {
        const int64_t SC = (int64_t)a.S * C;          // floats of v per (pass, input row)
        if (SC <= LDS_FLOATS) {
            a.SCH = a.S;
            a.RB = SC >= WNT ? 1 : (int)(WNT / SC);
            a.SEG = a.RB * (int)SC;
            a.WBS = LDS_FLOATS / a.SEG < WBMAX ? LDS_FLOATS / a.SEG : WBMAX;
        } else {                                      // one pass of one row per round, in chunks of SCH paths
            a.SCH = LDS_FLOATS / C; a.RB = 1; a.SEG = a.SCH * C; a.WBS = 1;
        }
        const int64_t rows = a.B / a.S;
        hipLaunchKernelGGL(snsde_cgrad_walk_groups_kernel, dim3((unsigned)((rows + a.RB - 1) / a.RB)), dim3(WNT),
                           (size_t)a.WBS * a.SEG * sizeof(float), stream, a);
    }
    else hipLaunchKernelGGL(snsde_cgrad_walk_kernel, dim3((unsigned)((BC + 63) / 64)), dim3(64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}
