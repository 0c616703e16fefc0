// Kernel templates, argument structs and per-configuration dispatch of the MFMA fast path (forward + adjoint).
// Included by snsde_mfma.hip (host side: plans, packing) and by one translation unit per hidden size
// (snsde_mfma_h*.hip), which are compiled in parallel.
#pragma once
//
// One persistent workgroup owns a tile of M batch rows for ALL solver steps.  Per step the MLP drift
// (neuralsde.py:295-302) is a chain of small GEMMs  out^T (features x rows) = W (features x K) . act^T,
// executed on the f32 matrix cores (exact f32: an MFMA is bit-for-bit an fmaf chain):
//
//   * every wave of the workgroup owns a slice of OUTPUT FEATURES of every layer and keeps that slice
//     of every weight matrix RESIDENT IN REGISTERS (VGPR+AGPR, one wave per SIMD, 512 registers/lane)
//     for the whole solve: zero weight traffic per step;
//   * weights are the MFMA A operand, activations the B operand ("transposed" product), so a batch row
//     stays in one lane column: the D fragment of a layer IS one 16-byte LDS store per lane, and the
//     next layer's B fragment is plain ds_read_b128 of the row-major LDS activation buffer (the k-slot
//     to feature assignment is arbitrary as long as A and B agree: k(u, s, e) = 16u + 4s + e);
//   * the state y, dW, f, g and the Euler/Milstein update live in registers in the D layout of the last
//     layer; the time-only diffusion MLP of noise_option 16/17 is a per-step table (hoisted);
//   * activations cross waves through padded LDS buffers (row stride = 8 or 16 mod 64 floats:
//     conflict-free ds_read_b128), one s_barrier per layer.
//
// Two tile flavours share the code:
//   M16: v_mfma_f32_16x16x4_f32, 16 rows per workgroup  (lane = 16*s + row).        Large batches.
//   M4 : v_mfma_f32_4x4x1_16b_f32, 4 rows per workgroup: the 16 independent 4x4 blocks are used as
//        4 k-slots x 4 feature quads (lane = 16*q + 4*s + row); the k-slot partial sums are combined by a
//        DPP reduce-scatter (lane s keeps feature 4q+s: one element per lane from there on), and the B operand
//        (a function of lane & 15 only) is read by lanes 0-15 and broadcast by the MFMA (blgp:4).
//        Fills all 256 CUs at batch 1024.
#include "snsde_internal.h"

namespace snsde_mfma {


typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int MAXL = 4 + SNSDE_MAX_HIDDEN;

struct MfmaLayerPack {
    int32_t src_w, src_b, K, tshift, N, KU, dst;  // dst = float offset of the packed fragment block
    // folding (emb o linear_in / emb o initial_network): the product emb[:, fold_col:fold_col+H] . src is formed
    // first by snsde_fold_kernel into a workspace temp (same (N, K) layout), which the pack kernel then reads
    int32_t fold, fold_w, fold_col, fold_ld, fold_tmp, bias_row;   // bias_row < 0: piece has no bias row
    // transpose (backward pass): packed row index = forward INPUT feature, k = forward OUTPUT feature:
    // value = src[k * src_ld + col_off + feat]  (src = params + src_w, or the folded product in ws + fold_tmp)
    int32_t transpose, src_ld, col_off;
    // lean M4 layout (snsde_m4_kernel.h): the `tshift` leading source columns (sin t, cos t) are not rotated to the end of
    // this layer's own k axis but written into ANOTHER packed block (the [X(t) | sin t, cos t] block) at columns t_col0..;
    // [hole0, hole1) = padding columns of this block that another piece writes (left untouched here)
    int32_t t_on, t_dst, t_KU, t_col0, hole0, hole1;
};

struct MfmaPackJob {
    MfmaLayerPack layer[MAXL];
    int32_t n_layers, flavor, TPW, NW, bias_off, H;
    int32_t fold_b_in, fold_b_init, fold_b_emb, fold_emb_w;   // folded bias = b_emb + E1 b_in + E2 b_init
    int32_t fold_bias_tmp;
};

// F = E[:, col:col+H] . W   (E = emb.weight (H, 2H), W = linear_in.weight (H, K) or initial_network.weight (H, C)),
// one block per output row f; lanes run over the K columns (coalesced reads of W rows).  Block y = piece.
struct FoldJob {
    int32_t emb_w, H, n_pieces;
    int32_t src_w[2], K[2], col[2], tmp[2];
    int32_t b_in, b_init, b_emb, bias_tmp;
    // time-only diffusion table built by the same launch (blockIdx.y == 2): gt[n][H] for n < n_steps
    int32_t tab_on, tab_off, n_steps, no, fold_on, off_sigma, off_sigma_diag;
    SnsdeLayer nt0, nt1;
    const float* step_tab;
    SnsdeZ0Job z0;      // initial state from the control path in the same launch (z0.w == nullptr: none)
};

struct MfmaArgs {
    const float* params;
    const float* ws;
    const float* coeffs;
    const float* step_tab;
    const int32_t* out_step;
    const float* out_w;
    const float* y0;
    const float* dW;
    const float* dU;   // SRK: supplied space-time Levy integrals I_k0 (with dW) or null
    float* dU_out;     // SRK: I_k0 used, or null
    float* ys;
    float* traj;
    float* dW_out;
    float* act_save;   // (N, NSAVE, B, H) or null
    float* stage_save; // SRK training: (3N + 1, B, H) input state of every drift pass, or null
    const int32_t* row_out;   // (B) per-row output slot (ys is then (B, H)) or null
    int64_t row_offset;
    uint64_t seed;
    const uint64_t* seed_dev;   // device-resident key (overrides seed) or null
    int32_t B, L, C, N, T, method, no;
    int32_t off_theta, gt_off, bias_off;
    int32_t w_off[MAXL];
    int32_t lean_xc, lean_time, lean_geo;   // lean M4 kernel: control channels in the xt block, time features on, z *= tanh(y)
    int32_t act, f_out, g_out, raw_time;    // field variants (include/snsde.h: SNSDE_ACT_*, SNSDE_DRIFT_*, SNSDE_DIFFUSION_*, SNSDE_TIME_*)
    const float* gt_ext;                    // caller-supplied time-only diffusion table (N, H) or null
    int32_t acc_col;                        // path-integral accumulator column (snsde_solve.kl_column1 - 1), -1: none
    float acc_a, acc_b;                     // its linear prior drift a y + b
    int32_t samples;                        // paths per input row, >= 1 (snsde_solve::samples): path p reads coeffs row p / samples;
                                            // read by the lean and the general kernel (make_plan refuses the others) and, for an
                                            // ensemble under SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_SAMPLES, by snsde_m4n_kernel
    // model ensembles (snsde_solve::members = M > 1): the member is the launch's second grid axis, m = blockIdx.y (one model: a
    // grid of one row, m = 0 and the strides are 0) - tile blockIdx.x of member m covers rows m member_rows + 4 blockIdx.x .., reads
    // params + m param_stride, ws + m ws_stride and coefficient rows counted from the member's first row.  No division and no branch:
    // a `row0 / member_rows` behind a uniform test put a dependent kernarg load in front of every other load of the prologue.  Read by
    // the lean kernel, the general kernel and - under SNSDE_FLAG_ENSEMBLE_NETS - snsde_m4n_kernel (make_plan refuses the others for
    // M > 1; the wave pairs carry the same three fields in W4Args), once per workgroup before the step loop
    int32_t members, member_rows;           // member_rows: rows per member (batch / M; one model: unused, m = 0)
    uint32_t param_stride, ws_stride;       // floats
    // resumed solves (snsde_solve_forward_at): local step n draws the normals of global step step_offset + n - Philox counter
    // (row_offset + row, (step_offset + n) >> 2, col, stream), element (step_offset + n) & 3.  Uniform (a kernel argument: scalar unit);
    // read at the Philox sites only - tables, outputs and saved planes stay indexed by the local step.  A kernel that keeps the normals
    // of a block (or a batch of blocks) fills, on its first step, the block (batch) that CONTAINS step_offset, whatever its phase
    int32_t step_offset;
};

__host__ __device__ constexpr int ld_for(int K, int pad) { return ((K - pad + 63) / 64) * 64 + pad; }

template <int FL> __device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    if constexpr (FL == 0) return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 4);   // BLGP 4: B taken from lanes 0-15 for every 16-lane group
}

// k-slot reduction of the M4 flavour: lanes 4s+j (s = 0..3) of every 16-lane row hold partial sums
__device__ __forceinline__ float row_ror_add(float x) {
    float a = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x124, 0xf, 0xf, false));
    x += a;
    float b = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xf, 0xf, false));
    return x + b;
}

// k-slot reduce-scatter of the M4 flavour: lane 16q+4s+r holds the partial sums v[0..3] (features 4q..4q+3, row r) of
// k-slot s; lane s gets back the total of v[s] over the four k-slots.  Butterfly over lane bit 3 (row_ror:8) and bit 2
// (row_ror:12 = from lane+4 / row_ror:4 = from lane-4); which half a lane keeps is selected by the DPP bank mask
// (bank = s), so there are no selects: 6 VALU ops (all-reduce of four values + select: 19).  The s_nops cover the
// VALU-write -> DPP-read hazard the assembler does not see inside inline asm.
__device__ __forceinline__ float m4_reduce_scatter(f32x4 v) {
    float z0 = v[0], z1 = v[1], z2 = v[2], z3 = v[3], a0, a1, r;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %1, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %1, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %2, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        : "=&v"(a0), "=&v"(a1), "=&v"(r)
        : "v"(z0), "v"(z1), "v"(z2), "v"(z3));
    return r;
}

// y-only closed-form diffusions (noise_option 7..10, neuralsde.py:250-261): raw = phi(y) with its first two derivatives
// 1 / g with |g| floored at 1e-7 (the reference's _stable_division, latent_sde.py:25-27)
__device__ __forceinline__ float snsde_stable_inv(float g) {
    const float gs = fabsf(g) > 1e-7f ? g : copysignf(1e-7f, g) * (g != 0.0f ? 1.0f : 0.0f);
    return 1.0f / gs;
}
// sum of v over the lanes of a 4-row-tile wave that share the batch row (lane & 3): the wave's 16 features
__device__ __forceinline__ float m4_row_sum(float v) {
    v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ float snsde_phi(int no, float y, float& r1, float& r2) {
    if (no == 7) { const float q = sqrtf(y); r1 = 0.5f / q; r2 = -0.25f / (q * y); return q; }
    if (no == 8) { r1 = 3.0f * y * y; r2 = 6.0f * y; return y * y * y; }
    if (no == 9) { const float q = snsde_sigmoid(y); r1 = q * (1.0f - q); r2 = r1 * (1.0f - 2.0f * q); return q; }
    r1 = y > 0.0f ? 1.0f : 0.0f; r2 = 0.0f;
    return fmaxf(y, 0.0f);
}

// tanh on the hardware exp2 / rcp units, branch-free:
//   |x| <  0.25 : odd Taylor polynomial to x^11 (truncation < 3e-10 relative)
//   |x| >= 0.25 : (1 - t) / (1 + t), t = 2^(-2 log2(e) |x|) in (0, 0.61]: no cancellation in 1 - t, the result
//                 carries <= ~3 ulp relative error; saturates to +-1, NaN preserved.
__device__ __forceinline__ float fast_tanh(float x) {
    const float ax = fabsf(x);
    const float x2 = x * x;
    float p = fmaf(x2, -0.0088632355299021967f, 0.021869488536155203f);   // -1382/155925, 62/2835
    p = fmaf(x2, p, -0.053968253968253971f);                              // -17/315
    p = fmaf(x2, p, 0.13333333333333333f);                                // 2/15
    p = fmaf(x2, p, -0.33333333333333333f);
    p = fmaf(x * x2, p, x);
    const float t = __builtin_amdgcn_exp2f(ax * -2.8853900817779268f);
    const float q = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
    return ax < 0.25f ? p : copysignf(q, x);
}

// Relu signs inside the saved pre-tanh drift (round 4).  The MFMA adjoint needs [activation > 0] of every rectified layer output of a
// step; it used to re-read the saved activation planes for that - two of the seven (N, B, H) planes a K2 adjoint step moves.  A lane
// owns the SAME (row, feature) element of every layer's output and of the drift output z, so the forward kernels fold the signs of that
// element's rectified outputs into the low mantissa bits of the z they save (snsde_save_layout.h: sign_bits) and the adjoint takes its
// masks from the z it loads anyway: no extra store, load or buffer.  The saved z is used for tanh'(z) only (its low <= 4 bits are noise of <= 1e-6 relative; the forward itself computes with
// the exact register value, so states are bit-identical); models with a smooth activation keep their pre-activation planes.
__device__ __forceinline__ float snsde_pack_signs(float z, uint32_t signs, int nbits) {
    const uint32_t m = (1u << nbits) - 1u;
    return __uint_as_float((__float_as_uint(z) & ~m) | (signs & m));
}

// Wave-uniform element offset  n * stride + slot * bh  from 32 x 32 -> 64-bit products (s_mul_i32 / s_mul_hi_u32 on the scalar unit).
// Written as 64 x 64-bit products of size_t values, hipcc evaluates them on the VALU (v_mad_u64_u32 + two quarter-rate v_mul_lo_u32
// per product) - ~25 of them per step in the adjoint loop, on the issue port the MFMAs share.  stride, bh < 2^32 (B H times the slots
// per step: checked by the launcher).
__device__ __forceinline__ size_t uoff(int n, uint32_t stride, uint32_t slot = 0, uint32_t bh = 0) {
    return (size_t)((uint64_t)(uint32_t)n * stride + (uint64_t)slot * bh);
}

template <int KU, int TPW>
__device__ __forceinline__ void load_weights(float (&w)[TPW][KU * 4], const float* __restrict__ g, int wave, int lane) {
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + (((wave * TPW + t) * KU + u) * 64 + lane) * 4);
            w[t][4 * u + 0] = v[0]; w[t][4 * u + 1] = v[1]; w[t][4 * u + 2] = v[2]; w[t][4 * u + 3] = v[3];
        }
}

// acc[t] += W_tile(t) . in   over KU blocks of 16 k;  `in` = this lane's LDS row pointer + 4*s
// Two interleaved accumulator chains per tile (acc / acc2, summed by the caller) keep dependent MFMAs apart.
template <int FL, int KU, int TPW>
__device__ __forceinline__ void gemm(const float (&w)[TPW][KU * 4], const float* in, f32x4 (&acc)[TPW],
                                     f32x4 (&acc2)[TPW]) {
    f32x4 b[KU];
    if constexpr (FL) {
        // M4: the B operand depends on (k-slot, row) = lane & 15 only, the MFMA broadcasts lanes 0-15 (BLGP 4): only those
        // lanes read LDS, a quarter of the LDS traffic of a full-wave ds_read_b128
#pragma unroll
        for (int u = 0; u < KU; ++u) asm volatile("" : "=v"(b[u]));     // lanes 16-63: whatever the registers hold (never read)
        if ((int)(threadIdx.x & 63) < 16) {
#pragma unroll
            for (int u = 0; u < KU; ++u) b[u] = *reinterpret_cast<const f32x4*>(in + 16 * u);
        }
    } else {
#pragma unroll
        for (int u = 0; u < KU; ++u) b[u] = *reinterpret_cast<const f32x4*>(in + 16 * u);
    }
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int e = 0; e < 4; e += 2)
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                acc[t] = mfma<FL>(w[t][4 * u + e], b[u][e], acc[t]);
                acc2[t] = mfma<FL>(w[t][4 * u + e + 1], b[u][e + 1], acc2[t]);
            }
}

// Where a wave's weight slice lives: registers for the whole solve (the default), or streamed from the packed
// workspace (L2-resident) every use when the matrices exceed the register file (H = 256).
template <bool STREAM, int KU, int TPW> struct Wt;
template <int KU, int TPW> struct Wt<false, KU, TPW> {
    float v[TPW][KU * 4];
    __device__ __forceinline__ void load(const float* __restrict__ g, int wave, int lane) { load_weights<KU, TPW>(v, g, wave, lane); }
};
template <int KU, int TPW> struct Wt<true, KU, TPW> {
    const float* p;   // this lane's first float4 of the wave's packed block
    __device__ __forceinline__ void load(const float* __restrict__ g, int wave, int lane) {
        p = g + (size_t)wave * TPW * KU * 256 + lane * 4;
    }
};

template <int FL, int KU, int TPW>
__device__ __forceinline__ void gemm(const Wt<false, KU, TPW>& w, const float* in, f32x4 (&acc)[TPW], f32x4 (&acc2)[TPW]) {
    gemm<FL, KU, TPW>(w.v, in, acc, acc2);
}

// streamed variant: per 16-wide k-block one coalesced 1 KiB global load (float4 per lane) feeds four MFMAs
template <int FL, int KU, int TPW>
__device__ __forceinline__ void gemm(const Wt<true, KU, TPW>& w, const float* in, f32x4 (&acc)[TPW], f32x4 (&acc2)[TPW]) {
    static_assert(TPW == 1, "streamed weights: one tile per wave");
    constexpr int CH = 4;   // k-blocks in flight
#pragma unroll
    for (int c0 = 0; c0 < KU; c0 += CH) {
        f32x4 wv[CH], bv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if (c0 + i < KU) {
                wv[i] = *reinterpret_cast<const f32x4*>(w.p + (size_t)(c0 + i) * 256);
                bv[i] = *reinterpret_cast<const f32x4*>(in + 16 * (c0 + i));
            }
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if (c0 + i < KU) {
                acc[0] = mfma<FL>(wv[i][0], bv[i][0], acc[0]);
                acc2[0] = mfma<FL>(wv[i][1], bv[i][1], acc2[0]);
                acc[0] = mfma<FL>(wv[i][2], bv[i][2], acc[0]);
                acc2[0] = mfma<FL>(wv[i][3], bv[i][3], acc2[0]);
            }
    }
}

// ---- streamed weights through a per-wave LDS ring (H = 256, 4-row tiles; forward: snsde_m4s_kernel.h, adjoint: the
//      STREAM && FL branch of snsde_mfma_reverse_kernel) ------------------------------------------------------------------
// LDS byte address of a __shared__ float
__device__ __forceinline__ uint32_t lean_lds_addr(const float* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const float*)(p);
}
// a wave-uniform pointer as an SGPR pair for "s" asm operands (readfirstlane folds away when hipcc knows it is uniform)
__device__ __forceinline__ uint64_t lean_uniform(const float* p) {
    const uint64_t v = (uint64_t)p;          // wave-uniform by construction; readfirstlane folds away when hipcc knows it
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// LDS-DMA of streamed k-block G (static): layer G / 16, block u = G % 16 of the wave's slice, into ring slot u % 8.
// Source = sb (the wave's slice of the layer, SGPR pair) + vo (lane * 16 + 4096 [+ 8192 for u >= 8]) + imm, imm =
// (u % 8) * 1024 - 4096; the immediate also moves the LDS destination (tools/ubench/glds_probe.hip), which therefore is
// M0 + imm + lane * 16 with M0 = ring base + 4096 for every slot.
template <int U>
__device__ __forceinline__ void stream_refill(uint32_t m0v, uint32_t vo_lo, uint32_t vo_hi, uint64_t sb) {
    constexpr int IMM = (U % 8) * 1024 - 4096;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %1, %2 offset:%3"
                 :: "s"(m0v), "v"(U < 8 ? vo_lo : vo_hi), "s"(sb), "n"(IMM) : "memory");
}

// One chunk: k-blocks U0, U0+1 of a layer.  B operands (lanes 0-15) from the activation row, wait for the chunk's ring
// slots (the R - 2 younger refills may stay in flight), A operands from the ring, refill the two slots, 8 MFMAs.
template <int U0, int BOFF>
__device__ __forceinline__ void stream_chunk(uint32_t baddr, uint32_t ra, uint32_t m0v, uint32_t vo_lo, uint32_t vo_hi,
                                             uint64_t sb_next, f32x4& c, f32x4& d) {
    f32x4 b0, b1, a0, a1;
    asm volatile("s_mov_b64 exec, 0xffff\n\t"
                 "ds_read_b128 %0, %[b] offset:%[o0]\n\tds_read_b128 %1, %[b] offset:%[o1]\n\t"
                 "s_mov_b64 exec, -1\n\t"
                 "s_waitcnt vmcnt(6)\n\t"
                 "ds_read_b128 %2, %[a] offset:%[s0]\n\tds_read_b128 %3, %[a] offset:%[s1]"
                 : "=&v"(b0), "=&v"(b1), "=&v"(a0), "=&v"(a1)
                 : [b] "v"(baddr), [a] "v"(ra), [o0] "n"(BOFF + U0 * 64), [o1] "n"(BOFF + U0 * 64 + 64),
                   [s0] "n"((U0 % 8) * 1024), [s1] "n"((U0 % 8) * 1024 + 1024)
                 : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b0), "+v"(b1), "+v"(a0), "+v"(a1));
    // the slots are free: their next tenants are blocks U0 + 8, U0 + 9 (same layer while U0 < 8, else the next streamed
    // layer's / next step's first blocks)
    stream_refill<(U0 + 8) % 16>(m0v, vo_lo, vo_hi, sb_next);
    stream_refill<(U0 + 9) % 16>(m0v, vo_lo, vo_hi, sb_next);
#define SNSDE_S4(av, bv) \
    c = __builtin_amdgcn_mfma_f32_4x4x1f32(av[0], bv[0], c, 0, 0, 4); d = __builtin_amdgcn_mfma_f32_4x4x1f32(av[1], bv[1], d, 0, 0, 4); \
    c = __builtin_amdgcn_mfma_f32_4x4x1f32(av[2], bv[2], c, 0, 0, 4); d = __builtin_amdgcn_mfma_f32_4x4x1f32(av[3], bv[3], d, 0, 0, 4);
    SNSDE_S4(a0, b0) SNSDE_S4(a1, b1)
#undef SNSDE_S4
    __builtin_amdgcn_sched_barrier(0);
}

// one streamed layer: sb = this layer's slice (the first half's chunks refill from it), sbn = the next streamed layer's;
// BOFF = byte offset of the layer's input rows from the y rows (same row stride)
template <int BOFF>
__device__ __forceinline__ void stream_layer(uint32_t baddr, uint32_t ra, uint32_t m0v, uint32_t vo_lo, uint32_t vo_hi,
                                             uint64_t sb, uint64_t sbn, f32x4& c, f32x4& d) {
    stream_chunk<0, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sb, c, d);
    stream_chunk<2, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sb, c, d);
    stream_chunk<4, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sb, c, d);
    stream_chunk<6, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sb, c, d);
    stream_chunk<8, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sbn, c, d);
    stream_chunk<10, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sbn, c, d);
    stream_chunk<12, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sbn, c, d);
    stream_chunk<14, BOFF>(baddr, ra, m0v, vo_lo, vo_hi, sbn, c, d);
}


template <int H_, int KUX_, int NHID_, int IO_, int FL_, int PHX_, int FOLD_, int NN_ = 0, int SRK_ = 0>
struct Cfg {
    static constexpr bool SRK = SRK_ != 0;   // SRID2 stepper: three drift passes (pseudo-steps) per solver step
    static constexpr int H = H_, KUX = KUX_, NHID = NHID_, IO = IO_, FL = FL_;
    // PHX_ (in-kernel Philox increments vs supplied dW) is decided at run time from a.dW: one instantiation serves both
    // (the template slot is kept at 1 by every dispatch)
    // one 16-feature tile per wave: H/16 waves per workgroup (8 at H=128 = two waves per SIMD, so one wave's
    // LDS/barrier/VALU latency hides under the other's MFMAs, and the 172 resident weight registers of a wave
    // fit the 256-register budget without AGPR round trips)
    static constexpr int TPW = 1;
    static constexpr int NW = H / (16 * TPW);
    static constexpr int WPS = NW >= 4 ? NW / 4 : 1;   // waves per SIMD
    static constexpr int NT = NW * 64;
    static constexpr int M = FL ? 4 : 16;
    static constexpr bool TIME = IO >= 3;
    static constexpr int NN = NN_;            // diffusion net on [tau, y]: 0 none, 1 = noise_y Linear (no 14/15), 2 = two layers (18/19)
    static constexpr bool YTIME = TIME || NN > 0;   // ybuf carries the [sin t, cos t] columns
    static constexpr bool EMB = (IO == 2 || IO == 4 || IO == 6);
    static constexpr bool IO0 = (IO == 0);            // drift on the control path only: z = initial_network(X(t))
    static constexpr bool USEX = EMB || IO0;          // the spline value X(t) is an input of the first layer
    static constexpr bool GEO = (IO == 5 || IO == 6);
    static constexpr bool STREAM = H > 128;   // weights streamed from L2 instead of register-resident
    static constexpr bool FOLD = EMB && FOLD_ != 0;   // emb o (linear_in, initial_network) pre-multiplied
    static constexpr int KUH = H / 16;
    static constexpr int KUY = KUH + (TIME ? 1 : 0);
    static constexpr int KUE = 2 * KUH;
    static constexpr int PAD = FL ? 16 : 8;
    static constexpr int KUN = KUH + 1;       // noise net input = [y, sin t, cos t]
    static constexpr int LDY = ld_for(16 * (YTIME ? KUH + 1 : KUH), PAD);
    static constexpr int LDX = ld_for(16 * KUX, PAD);
    static constexpr int LDC = FOLD ? 0 : ld_for(EMB ? 32 * KUH : 16 * KUH, PAD);   // folded first layer needs no concat buffer
    static constexpr int LDA = ld_for(16 * KUH, PAD);
    static constexpr int NLAYER = (EMB && !FOLD ? 3 : 1) + NHID + 1 + NN;   // bias rows: [init, in, emb] | [first], hid.., out, noise..
    static constexpr int XI = (M * 16 * KUX + NT - 1) / NT;           // spline items per thread
    static constexpr int EPT = FL ? 1 : 4;                            // owned state elements per lane per tile
    static constexpr int NSAVE = snsde_save::act_slots(NHID, NN, SRK ? SNSDE_SRK : SNSDE_EULER);      // act_save slots per pass (snsde_save_layout.h)
    static constexpr int ZSLOT = snsde_save::act_z(NHID);
    static constexpr int ZB = (FL && !STREAM && !SRK) ? 4 : 1;                     // Philox calls generated together per element
    static constexpr int ROWCH = 128;                                 // step-table rows staged in LDS per chunk
    static constexpr int ZSTASH = !SRK ? 4 * ZB * 64 * EPT : 0;  // floats per wave (Philox normals of 4*ZB steps)
    static constexpr int LDS_BASE = M * (LDY + LDX + LDC + 3 * LDA) + NLAYER * H + (ROWCH + 1) * SNSDE_STEP_STRIDE;
    static constexpr int LDS_FLOATS = LDS_BASE + NW * ZSTASH;    // the Philox stash (last region) only when increments are generated
};

// Optional cycle trace (debug builds with -DSNSDE_TRACE): per-phase s_memtime deltas of every wave of block 0,
// accumulated over the steps and written over dW_out[wave*16 + phase] at the end (dW_out then holds no increments).
#ifdef SNSDE_TRACE
#define TRACE_DECL unsigned long long tr_t = __builtin_readcyclecounter(); unsigned long long tr_acc[10] = {0,0,0,0,0,0,0,0,0,0};
#define TRACE(i) { const unsigned long long tr_n = __builtin_readcyclecounter(); tr_acc[i] += tr_n - tr_t; tr_t = tr_n; }
#else
#define TRACE_DECL
#define TRACE(i)
#endif

template <class CF>
__global__ void __launch_bounds__(CF::NT, CF::WPS) snsde_mfma_kernel(MfmaArgs a) {
    constexpr int H = CF::H, TPW = CF::TPW, FL = CF::FL, M = CF::M, NT = CF::NT, NHID = CF::NHID;
    constexpr int KUX = CF::KUX, KUY = CF::KUY, KUE = CF::KUE, KUH = CF::KUH, EPT = CF::EPT;
    constexpr int LDY = CF::LDY, LDX = CF::LDX, LDC = CF::LDC, LDA = CF::LDA;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ybuf = lds;                   // [M][LDY]  y (H) | sin t, cos t | 0..
    float* xbuf = ybuf + M * LDY;        // [M][LDX]  X(t) (C) | 0..
    float* cat = xbuf + M * LDX;         // [M][LDC]  yy (H) | Xt (H)        (or layer buffer when no emb)
    float* bufA = cat + M * LDC;         // [M][LDA]
    float* bufB = bufA + M * LDA;        // [M][LDA]
    float* nbuf = bufB + M * LDA;        // [M][LDA]  hidden layer of the diffusion net (noise_option 18/19)
    float* bias = nbuf + M * LDA;        // [NLAYER][H]
    float* rowtab = bias + CF::NLAYER * H;   // [ROWCH + 1][SNSDE_STEP_STRIDE]
    float* zstash_all = rowtab + (CF::ROWCH + 1) * SNSDE_STEP_STRIDE;   // [NW][4*ZB][64][EPT] per-wave normals

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = FL ? (lane & 3) : (lane & 15);          // batch row within the tile
    const int s = FL ? ((lane >> 2) & 3) : (lane >> 4);   // k-slot
    const int fsub = FL ? 4 * (lane >> 4) : 4 * s;        // first feature (within a 16-feature tile) of the D fragment
    // model ensembles: blockIdx.y is the member (MfmaArgs::members; one model: 0) - its first row, its parameter and workspace blocks
    const uint32_t mem = blockIdx.y;
    const int mrow0 = (int)mem * a.member_rows;
    const int row0 = mrow0 + blockIdx.x * M;
    const float* const params = a.params + (size_t)mem * a.param_stride;
    const float* const ws = a.ws + (size_t)mem * a.ws_stride;
    float* zstash = zstash_all + wave * CF::ZSTASH;
    const int B = a.B, C = a.C;
    const int row = row0 + r;
    const int rowc = row < B ? row : B - 1;
    const bool row_ok = row < B;
    const size_t BH = (size_t)B * H;

    // ---- resident weights ----------------------------------------------------------------------
    int li = 0;
    Wt<CF::STREAM, CF::USEX ? KUX : 1, TPW> wx;
    Wt<CF::STREAM, KUY, TPW> wy;
    Wt<CF::STREAM, (CF::EMB && !CF::FOLD) ? KUE : 1, TPW> we;
    Wt<CF::STREAM, KUH, TPW> wh[(NHID > 0) ? NHID : 1];
    Wt<CF::STREAM, KUH, TPW> wo;
    Wt<CF::STREAM, (CF::NN > 0) ? CF::KUN : 1, TPW> wn0;
    Wt<CF::STREAM, (CF::NN > 1) ? KUH : 1, TPW> wn1;
    if constexpr (CF::USEX) wx.load(ws + a.w_off[li++], wave, lane);
    if constexpr (!CF::IO0) wy.load(ws + a.w_off[li++], wave, lane);
    if constexpr (CF::EMB && !CF::FOLD) we.load(ws + a.w_off[li++], wave, lane);
#pragma unroll
    for (int l = 0; l < NHID; ++l) wh[l].load(ws + a.w_off[li++], wave, lane);
    wo.load(ws + a.w_off[li++], wave, lane);
    if constexpr (CF::NN > 0) wn0.load(ws + a.w_off[li++], wave, lane);
    if constexpr (CF::NN > 1) wn1.load(ws + a.w_off[li++], wave, lane);

    // ---- LDS init ------------------------------------------------------------------------------
    for (int i = tid; i < M * (LDY + LDX + LDC + 3 * LDA); i += NT) lds[i] = 0.0f;
    for (int i = tid; i < CF::NLAYER * H; i += NT) bias[i] = ws[a.bias_off + i];
    __syncthreads();

    const float sig_theta = snsde_sigmoid(params[a.off_theta]);
    const int no = a.no;
    const float* gt = a.gt_ext ? a.gt_ext : ws + a.gt_off;     // (a caller-supplied time-only table: field variants)

    // owned state: tile t covers features 32*wave.. ; element e of this lane = feature f0(t) + fsub + (FL ? s : e)
    float yv[TPW][EPT];
    int fcol[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        fcol[t] = (wave * TPW + t) * 16 + fsub + (FL ? s : 0);
        if constexpr (FL) {
            yv[t][0] = a.y0[(size_t)rowc * H + fcol[t]];
            ybuf[r * LDY + fcol[t]] = yv[t][0];
            if (row_ok) {
                a.ys[(size_t)row * H + fcol[t]] = yv[t][0];
                if (a.traj) a.traj[(size_t)row * H + fcol[t]] = yv[t][0];
                if constexpr (CF::SRK) { if (a.stage_save) a.stage_save[(size_t)row * H + fcol[t]] = yv[t][0]; }
            }
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.y0 + (size_t)rowc * H + fcol[t]);
            yv[t][0] = v[0]; yv[t][1] = v[1]; yv[t][2] = v[2]; yv[t][3] = v[3];
            *reinterpret_cast<f32x4*>(ybuf + r * LDY + fcol[t]) = v;
            if (row_ok) {
                *reinterpret_cast<f32x4*>(a.ys + (size_t)row * H + fcol[t]) = v;
                if (a.traj) *reinterpret_cast<f32x4*>(a.traj + (size_t)row * H + fcol[t]) = v;
                if constexpr (CF::SRK) { if (a.stage_save) *reinterpret_cast<f32x4*>(a.stage_save + (size_t)row * H + fcol[t]) = v; }
            }
        }
    }

    // spline items of this thread: (xr, xc) = row-in-tile, channel
    // (xs: the coeffs row of the item - the path's row, ragged tail clamped, over the paths per input row)
    int xr[CF::XI], xc[CF::XI], xs[CF::XI];
    bool xok[CF::XI];
    float ca[CF::XI], cb[CF::XI], cc[CF::XI], cd[CF::XI];
#pragma unroll
    for (int i = 0; i < CF::XI; ++i) {
        const int it = tid + i * NT;
        xr[i] = it / C; xc[i] = it - xr[i] * C;
        xok[i] = CF::USEX && it < M * C;
        if (!xok[i]) { xr[i] = 0; xc[i] = 0; }
        const int rp = (row0 + xr[i] < B ? row0 + xr[i] : B - 1) - mrow0;
        xs[i] = a.samples > 1 ? (int)((uint32_t)rp / (uint32_t)a.samples) : rp;
    }
    auto load_coeffs = [&](int idx) {
#pragma unroll
        for (int i = 0; i < CF::XI; ++i) {
            if (xok[i]) {
                const int rr = xs[i];
                const float* cp = a.coeffs + ((size_t)rr * (a.L - 1) + idx) * (4 * C) + xc[i];
                ca[i] = cp[0]; cb[i] = cp[C]; cc[i] = cp[2 * C]; cd[i] = cp[3 * C];
            }
        }
    };
    auto store_x = [&](float frac) {
#pragma unroll
        for (int i = 0; i < CF::XI; ++i)
            if (xok[i]) xbuf[xr[i] * LDX + xc[i]] = snsde_spline_eval(ca[i], cb[i], cc[i], cd[i], frac);
    };
    {   // step 0 inputs
        const float* st = a.step_tab;
        if constexpr (CF::USEX) { load_coeffs(__float_as_int(st[5])); store_x(st[4]); }
        if (CF::YTIME && tid < M) { ybuf[tid * LDY + H] = st[2]; ybuf[tid * LDY + H + 1] = st[3]; }
    }
    __syncthreads();

    const float* yrow = ybuf + r * LDY + 4 * s;
    const float* xrow = xbuf + r * LDX + 4 * s;
    const float* crow = cat + r * LDC + 4 * s;
    const float* arow = bufA + r * LDA + 4 * s;
    const float* brow = bufB + r * LDA + 4 * s;
    const bool writer = FL ? (s == 0) : true;
    const bool mul_y = (no == 13 || no == 17 || no == 15 || no == 19 || no == 3 || no == 6 || no == 11);
    const bool yfun = (no >= 7 && no <= 10);     // raw = phi(y)
    const float mil = (a.method == SNSDE_MILSTEIN) ? 0.5f : 0.0f;
    const uint32_t grow = (uint32_t)(a.row_offset + row);
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
    const int rslot = a.row_out ? a.row_out[rowc] : -1;     // per-row output selection (ys is (B, H))
    const bool phx = a.dW == nullptr;                       // in-kernel Philox increments (else the supplied ones)
    const int n0 = a.step_offset;                           // resumed solves: the global index of local step 0 (MfmaArgs)

    // store one layer output fragment (bias came in through the accumulator init) as 16 B per lane
    int save_step = 0;   // current step, for the optional activation save
    // relu signs of this lane's elements of the step's rectified layers (snsde_pack_signs): bit (slot) on 4-row tiles, bit
    // (slot + 8 i) for fragment element i on 16-row tiles; folded into the saved z and cleared at the end of the step / SRK pass
    [[maybe_unused]] uint32_t sgn = 0;
    const bool pack_signs = a.act == 0 && a.act_save != nullptr;      // (SRK: every pass's z carries the pass's signs)
    // field variants with a smooth activation (4-row tiles; with a diffusion net they run snsde_m4n_kernel.h): + the pre-activations
    const int nsave_rt = (FL && a.act != 0) ? CF::NSAVE + snsde_save::pre_slots(NHID, 0, SNSDE_EULER, true) : CF::NSAVE;
    // M4: the layer's bias is added after the k-slot reduction, from a register (one value per lane and layer)
    float bias_own[CF::NLAYER];
#pragma unroll
    for (int l = 0; l < CF::NLAYER; ++l) bias_own[l] = FL ? ws[a.bias_off + l * H + wave * 16 + fsub + s] : 0.0f;
    auto finish = [&](int lyr, f32x4 v) { return m4_reduce_scatter(v) + bias_own[lyr]; };   // M4: this lane's output
    auto store_frag = [&](float* buf, int ld, int col0, f32x4 v, bool relu, int save_slot, int lyr) {
        if constexpr (FL) {
            float o = finish(lyr, v);
            const float pre = o;
            if (relu) {
                if (__builtin_expect(a.act != 0, 0)) {     // field variants (SRK of the tutorial-style fields): LipSwish / SiLU
                    const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(o * -1.4426950408889634f));
                    o = (a.act == SNSDE_ACT_LIPSWISH ? 0.909f : 1.0f) * o * sg;
                } else {
                    o = fmaxf(o, 0.0f);
                }
            }
            buf[r * ld + col0 + fsub + s] = o;
            if (relu && save_slot >= 0 && save_slot <= NHID) sgn |= (o > 0.0f ? 1u : 0u) << save_slot;
            if (save_slot >= 0 && a.act_save && row_ok) {
                (a.act_save + uoff(save_step, (uint32_t)nsave_rt * (uint32_t)(B * H), save_slot, (uint32_t)(B * H)))[(uint32_t)(row * H + wave * 16 + fsub + s)] = o;
                if (relu && a.act != 0)      // smooth activations: the pre-activation as well (slots behind the regular ones)
                    (a.act_save + uoff(save_step, (uint32_t)nsave_rt * (uint32_t)(B * H), CF::NSAVE + save_slot, (uint32_t)(B * H)))[(uint32_t)(row * H + wave * 16 + fsub + s)] = pre;
            }
            return;
        }
        if (relu) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.0f);
            if (save_slot >= 0 && save_slot <= NHID) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sgn |= (v[i] > 0.0f ? 1u : 0u) << (save_slot + 8 * i);
            }
        }
        if (writer) {
            *reinterpret_cast<f32x4*>(buf + r * ld + col0 + fsub) = v;
            if (save_slot >= 0 && a.act_save && row_ok)
                *reinterpret_cast<f32x4*>(a.act_save + (((size_t)save_step * CF::NSAVE + save_slot) * B + row) * H +
                                          wave * 16 + fsub) = v;
        }
    };
    auto bias_frag = [&](int layer, int t) {
        if constexpr (FL) return f32x4{0.f, 0.f, 0.f, 0.f};
        return *reinterpret_cast<const f32x4*>(bias + layer * H + (wave * TPW + t) * 16 + fsub);
    };

    // Step-table rows are staged in LDS in chunks of ROWCH steps (a uniform global load per step would put its
    // whole latency on the step's critical path: the row feeds scalar control flow and the coefficient addresses).
    struct Row { float h, sn, cs, frac, sqh; int idx, nout, kfirst; };
    auto fill_rows = [&](int base) {
        for (int i = tid; i < (CF::ROWCH + 1) * SNSDE_STEP_STRIDE; i += NT) {
            const int rr = base + i / SNSDE_STEP_STRIDE;
            const int last = (CF::SRK ? 3 * a.N : a.N) - 1;
            rowtab[i] = a.step_tab[(size_t)(rr < last ? rr : last) * SNSDE_STEP_STRIDE + i % SNSDE_STEP_STRIDE];
        }
    };
    auto get_row = [&](int i, int base) {
        const float* st = rowtab + (i - base) * SNSDE_STEP_STRIDE;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(st), v1 = *reinterpret_cast<const f32x4*>(st + 4),
                    v2 = *reinterpret_cast<const f32x4*>(st + 8);
        Row q;
        q.h = v0[1]; q.sn = v0[2]; q.cs = v0[3]; q.frac = v1[0]; q.sqh = v1[2];
        q.idx = __float_as_int(v1[1]); q.nout = __float_as_int(v2[0]); q.kfirst = __float_as_int(v2[1]);
        return q;
    };
    fill_rows(0);
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(tid) >= NT / 2 && CF::NW >= 8) __builtin_amdgcn_s_setprio(1);   // younger half

    // SRK (SRID2): every solver step is three pseudo-steps of this loop (one drift pass each: stage times t0, t0 + h,
    // t0 + h/2 from the expanded step table); the stage combinations are elementwise in the D layout.
    float sk_y[EPT], sk_f0[EPT], sk_f1[EPT], sk_g0[EPT], sk_g1[EPT], sk_dw[EPT], sk_du[EPT];
    float sk_t0[EPT], sk_t1[EPT], sk_t3[EPT], sk_z[EPT][4], sk_x[EPT][4];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        sk_y[e] = yv[0][e]; sk_f0[e] = sk_f1[e] = sk_g0[e] = sk_g1[e] = sk_dw[e] = sk_du[e] = 0.0f;
        sk_t0[e] = sk_t1[e] = sk_t3[e] = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { sk_z[e][i] = 0.0f; sk_x[e][i] = 0.0f; }
    }
    const int n_loop = CF::SRK ? 3 * a.N : a.N;

    TRACE_DECL
    Row row_next = get_row(0, 0);
    for (int n = 0; n < n_loop; ++n) {
        TRACE(0)
        const bool more = n + 1 < n_loop;
        const int stage = CF::SRK ? n % 3 : 0;     // pseudo-step -> (solver step ns, stage)
        const int ns = CF::SRK ? n / 3 : n;
        save_step = n;
        const int rbase = (n / CF::ROWCH) * CF::ROWCH;
        if (n > 0 && n == rbase) {       // next chunk (every wave is past the previous step's closing barrier)
            fill_rows(rbase);
            __syncthreads();
        }
        const Row cur_row = row_next, nxt = get_row(more ? n + 1 : n, rbase);      // (row n was read as `nxt` by the previous pass)
        row_next = nxt;
        const float n_sin = nxt.sn, n_cos = nxt.cs, n_frac = nxt.frac;
        const int n_idx = nxt.idx;
        const int c_nout = cur_row.nout, c_kfirst = cur_row.kfirst;
        if constexpr (CF::USEX) { if (more) load_coeffs(n_idx); }   // prefetch next interval's cubic pieces
        const float h = cur_row.h, sqh = cur_row.sqh;

        // y-independent work of the step (Brownian increments, diffusion table row, next step's X(t) and time
        // features): done by every wave after the first layer's barrier (the first layer has read xbuf / the time
        // features of THIS step by then).  Splitting it between the two waves of a SIMD (older half before the hidden
        // GEMM, younger half after it) measured 1 % slower once the M4 B-operand reads were quartered.
        float dw[TPW][EPT];
        float gtv[TPW][EPT];
        auto prep = [&]() {
            // Brownian increments for the owned elements: one Philox call per (row, 4-step block, column) gives the
            // element's normals for 4 consecutive steps (snsde_philox_normal4), regenerated every 4th step
            static_assert(TPW == 1, "one 16-feature tile per wave");
            if constexpr (CF::SRK) {
                if (stage == 0) {      // increments (I_k, I_k0) and the diffusion table rows of the step's three stage times
#pragma unroll
                    for (int e = 0; e < EPT; ++e) {
                        if (phx) {
                            const int gs = n0 + ns, k = gs & 3;      // global step (resumed solves); the first step fills its block whatever its phase
                            if (k == 0 || n == 0) {
                                snsde_philox_normal4(seed, grow, (uint32_t)(gs >> 2), (uint32_t)(fcol[0] + e), sk_z[e], 0u);
                                snsde_philox_normal4(seed, grow, (uint32_t)(gs >> 2), (uint32_t)(fcol[0] + e), sk_x[e], 1u);
                            }
                            const float z = k == 0 ? sk_z[e][0] : (k == 1 ? sk_z[e][1] : (k == 2 ? sk_z[e][2] : sk_z[e][3]));
                            const float xi = k == 0 ? sk_x[e][0] : (k == 1 ? sk_x[e][1] : (k == 2 ? sk_x[e][2] : sk_x[e][3]));
                            sk_dw[e] = z * sqh;
                            sk_du[e] = h * fmaf(sqrtf(h / 12.0f), xi, 0.5f * sk_dw[e]);
                        } else {
                            const size_t off = (size_t)ns * BH + (size_t)rowc * H + fcol[0] + e;
                            sk_dw[e] = a.dW[off];
                            sk_du[e] = a.dU[off];
                        }
                        if (a.gt_off >= 0 || a.gt_ext) {
                            const float* gp = gt + (size_t)ns * 4 * H + fcol[0] + e;
                            sk_t0[e] = gp[0]; sk_t1[e] = gp[H]; sk_t3[e] = gp[3 * H];
                        }
                    }
                }
            } else if (phx) {
                // ZB independent Philox calls (ZB blocks of 4 steps) are generated together (their round chains interleave)
                // and parked in this wave's private LDS stash [4*ZB steps][64 lanes][EPT]; each step reads back one entry.
                // (resumed solves: batches are cut on the GLOBAL step n0 + n; the first step fills the batch that contains it)
                constexpr int ZB = CF::ZB;
                const int gn = n0 + n, k = (int)((uint32_t)gn % (uint32_t)(4 * ZB));
                if (k == 0 || n == 0) {
                    float zq[EPT][4 * ZB];
    #pragma unroll
                    for (int e = 0; e < EPT; ++e)
    #pragma unroll
                        for (int bb = 0; bb < ZB; ++bb)
                            snsde_philox_normal4(seed, grow, (uint32_t)(((gn - k) >> 2) + bb), (uint32_t)(fcol[0] + e), &zq[e][4 * bb]);
    #pragma unroll
                    for (int i = 0; i < 4 * ZB; ++i) {
                        if constexpr (FL) zstash[i * 64 + lane] = zq[0][i];
                        else *reinterpret_cast<f32x4*>(zstash + (i * 64 + lane) * 4) = f32x4{zq[0][i], zq[1][i], zq[2][i], zq[3][i]};
                    }
                }
                if constexpr (FL) dw[0][0] = zstash[k * 64 + lane] * sqh;
                else {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(zstash + (k * 64 + lane) * 4);
                    dw[0][0] = v[0] * sqh; dw[0][1] = v[1] * sqh; dw[0][2] = v[2] * sqh; dw[0][3] = v[3] * sqh;
                }
            } else {
                if constexpr (FL) dw[0][0] = a.dW[(size_t)n * BH + (size_t)rowc * H + fcol[0]];
                else {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(a.dW + (size_t)n * BH + (size_t)rowc * H + fcol[0]);
                    dw[0][0] = v[0]; dw[0][1] = v[1]; dw[0][2] = v[2]; dw[0][3] = v[3];
                }
            }
            // time-only diffusion table row (noise_option 12/13/16/17)
            if constexpr (!CF::SRK) {
    #pragma unroll
                for (int t = 0; t < TPW; ++t)
    #pragma unroll
                    for (int e = 0; e < EPT; ++e) gtv[t][e] = (a.gt_off >= 0) ? gt[(size_t)n * H + fcol[t] + e] : 0.0f;
            }


            if (more) {
                if constexpr (CF::USEX) store_x(n_frac);
                if (CF::YTIME && tid < M) { ybuf[tid * LDY + H] = n_sin; ybuf[tid * LDY + H + 1] = n_cos; }
            }
        };
        TRACE(1)
        f32x4 acc[TPW], acc2[TPW];
        f32x4 gnv = {0.f, 0.f, 0.f, 0.f};   // diffusion-net output fragment (noise_option 14/15/18/19)
        int layer = 0;
        auto init_acc = [&](int lyr) {
#pragma unroll
            for (int t = 0; t < TPW; ++t) { acc[t] = bias_frag(lyr, t); acc2[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        };
        auto sum_acc = [&]() {
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[t] += acc2[t];
        };
        // ---- drift: [init, in] -> emb -> hidden.. -> out   (FOLD: [emb o in | emb o init] -> hidden.. -> out) ----
        const float* cur;
        if constexpr (CF::FOLD) {
            init_acc(layer);
            gemm<FL, KUY, TPW>(wy, yrow, acc, acc2);
            gemm<FL, CF::EMB ? KUX : 1, TPW>(wx, xrow, acc, acc2);
            sum_acc();
            TRACE(2)
#pragma unroll
            for (int t = 0; t < TPW; ++t) store_frag(bufA, LDA, (wave * TPW + t) * 16, acc[t], true, 0, layer);
            ++layer;
            if constexpr (CF::NN > 0) {   // diffusion net, first layer, on the same [y, sin t, cos t] rows
                constexpr int NROW = CF::NLAYER - CF::NN;
                init_acc(NROW);
                gemm<FL, (CF::NN > 0) ? CF::KUN : 1, TPW>(wn0, yrow, acc, acc2);
                sum_acc();
                if constexpr (CF::NN == 2) store_frag(nbuf, LDA, wave * 16, acc[0], true, snsde_save::act_net(NHID, 0), NROW);
                else {
                    gnv = acc[0];
                    if constexpr (FL) {
                        gnv[0] = finish(NROW, gnv);
                        if (a.act_save && row_ok)
                            a.act_save[(((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 0)) * B + row) * H + wave * 16 + fsub + s] = gnv[0];
                    } else if (a.act_save && row_ok)
                        *reinterpret_cast<f32x4*>(a.act_save + (((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 0)) * B + row) * H + wave * 16 + fsub) = gnv;
                }
            }
            TRACE(3)
            __syncthreads();
            TRACE(4)
            if constexpr (CF::NN == 2) {   // second layer of the diffusion net (relu'd raw value, neuralsde.py:278-281)
                init_acc(CF::NLAYER - 1);
                gemm<FL, (CF::NN > 1) ? KUH : 1, TPW>(wn1, nbuf + r * LDA + 4 * s, acc, acc2);
                sum_acc();
                gnv = acc[0];
                if constexpr (FL) {
                    gnv[0] = fmaxf(finish(CF::NLAYER - 1, gnv), 0.0f);
                    if (a.act_save && row_ok)
                        a.act_save[(((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 1)) * B + row) * H + wave * 16 + fsub + s] = gnv[0];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) gnv[i] = fmaxf(gnv[i], 0.0f);
                    if (a.act_save && row_ok)
                        *reinterpret_cast<f32x4*>(a.act_save + (((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 1)) * B + row) * H + wave * 16 + fsub) = gnv;
                }
            }
            cur = arow;
        } else {
            if constexpr (CF::EMB) {
                init_acc(layer);
                gemm<FL, CF::EMB ? KUX : 1, TPW>(wx, xrow, acc, acc2);
                sum_acc();
#pragma unroll
                for (int t = 0; t < TPW; ++t) store_frag(cat, LDC, H + (wave * TPW + t) * 16, acc[t], false, -1, layer);
                ++layer;
            }
            init_acc(layer);
            if constexpr (CF::IO0) gemm<FL, CF::USEX ? KUX : 1, TPW>(wx, xrow, acc, acc2);      // z0 = initial_network(X(t))
            else gemm<FL, KUY, TPW>(wy, yrow, acc, acc2);
            sum_acc();
#pragma unroll
            for (int t = 0; t < TPW; ++t) store_frag(cat, LDC, (wave * TPW + t) * 16, acc[t], !CF::EMB, CF::EMB ? -1 : 0, layer);
            ++layer;
            if constexpr (CF::NN > 0) {   // diffusion net, first layer, on the same [y, sin t, cos t] rows
                constexpr int NROW = CF::NLAYER - CF::NN;
                init_acc(NROW);
                gemm<FL, (CF::NN > 0) ? CF::KUN : 1, TPW>(wn0, yrow, acc, acc2);
                sum_acc();
                if constexpr (CF::NN == 2) store_frag(nbuf, LDA, wave * 16, acc[0], true, snsde_save::act_net(NHID, 0), NROW);
                else {
                    gnv = acc[0];
                    if constexpr (FL) {
                        gnv[0] = finish(NROW, gnv);
                        if (a.act_save && row_ok)
                            a.act_save[(((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 0)) * B + row) * H + wave * 16 + fsub + s] = gnv[0];
                    } else if (a.act_save && row_ok)
                        *reinterpret_cast<f32x4*>(a.act_save + (((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 0)) * B + row) * H + wave * 16 + fsub) = gnv;
                }
            }
            __syncthreads();
            if constexpr (CF::NN == 2) {   // second layer of the diffusion net (relu'd raw value, neuralsde.py:278-281)
                init_acc(CF::NLAYER - 1);
                gemm<FL, (CF::NN > 1) ? KUH : 1, TPW>(wn1, nbuf + r * LDA + 4 * s, acc, acc2);
                sum_acc();
                gnv = acc[0];
                if constexpr (FL) {
                    gnv[0] = fmaxf(finish(CF::NLAYER - 1, gnv), 0.0f);
                    if (a.act_save && row_ok)
                        a.act_save[(((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 1)) * B + row) * H + wave * 16 + fsub + s] = gnv[0];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) gnv[i] = fmaxf(gnv[i], 0.0f);
                    if (a.act_save && row_ok)
                        *reinterpret_cast<f32x4*>(a.act_save + (((size_t)n * CF::NSAVE + snsde_save::act_net(NHID, 1)) * B + row) * H + wave * 16 + fsub) = gnv;
                }
            }
            cur = crow;
            if constexpr (CF::EMB) {
                init_acc(layer);
                gemm<FL, (CF::EMB && !CF::FOLD) ? KUE : 1, TPW>(we, crow, acc, acc2);
                sum_acc();
#pragma unroll
                for (int t = 0; t < TPW; ++t) store_frag(bufA, LDA, (wave * TPW + t) * 16, acc[t], true, 0, layer);
                ++layer;
                __syncthreads();
                cur = arow;
            }
        }
        prep();
#pragma unroll
        for (int l = 0; l < NHID; ++l) {
            // ping-pong: (emb|fold) -> A -> B -> A ... ; no-emb: cat -> A -> B ...
            const bool toB = CF::EMB ? (l % 2 == 0) : (l % 2 == 1);
            init_acc(layer);
            gemm<FL, KUH, TPW>(wh[l], cur, acc, acc2);
            sum_acc();
            TRACE(5)
#pragma unroll
            for (int t = 0; t < TPW; ++t) store_frag(toB ? bufB : bufA, LDA, (wave * TPW + t) * 16, acc[t], true, 1 + l, layer);
            ++layer;
            __syncthreads();
            TRACE(6)
            cur = toB ? brow : arow;
        }
        init_acc(layer);
        gemm<FL, KUH, TPW>(wo, cur, acc, acc2);
        sum_acc();

        TRACE(7)
        // ---- f, g, update in the D layout ----
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            f32x4 zv = acc[t];
            if constexpr (FL) zv[0] = finish(layer, zv);
            float ynew[EPT], yold[EPT], zsave[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                float z = zv[FL ? 0 : e];
                zsave[e] = z;
                const float y = yv[t][e];
                if constexpr (CF::GEO) z *= fast_tanh(y);
                float f = fast_tanh(z);
                if constexpr (CF::SRK) {
                    // field variants (tutorial-style fields): f = z or z * (the pass's input state), g = raw
                    if (__builtin_expect(a.f_out != 0, 0)) f = a.f_out == SNSDE_DRIFT_TIMES_Y ? z * y : z;
                    if constexpr (FL && CF::NN == 0) {
                        // path-integral accumulator column (snsde.h: kl_column1): its drift at this pass's (t, H0) is the KL rate
                        // u = 1/2 sum_j ((f_j - a y_j - b) / g_j)^2 over the latent columns j < acc_col - a sum over the tile row,
                        // i.e. over the lanes of every wave: per-wave row sums through LDS (nbuf is free without a diffusion net),
                        // one more barrier per pass; the owner lane takes u as ITS drift value and the scheme does the rest
                        if (__builtin_expect(a.acc_col >= 0, 0)) {
                            float ev = 0.0f;
                            if (fcol[t] < a.acc_col) {
                                const float q = (f - fmaf(a.acc_a, y, a.acc_b)) * snsde_stable_inv(sk_t0[e]);
                                ev = 0.5f * q * q;
                            }
                            ev = m4_row_sum(ev);
                            if (lane < 4) nbuf[wave * 4 + lane] = ev;
                            __syncthreads();
                            if (fcol[t] == a.acc_col) {
                                float u = 0.0f;
                                for (int w = 0; w < CF::NW; ++w) u += nbuf[w * 4 + r];
                                f = u;
                            }
                        }
                    }
                    auto gfun = [&](float gq, float yy) {
                        float q1, q2;
                        const float raw = yfun ? snsde_phi(no, yy, q1, q2) : (mul_y ? gq * yy : gq);
                        if (__builtin_expect(a.g_out != 0, 0)) return raw;
                        return fast_tanh(sig_theta * snsde_nan_to_num(raw));
                    };
                    const float yb = sk_y[e], f0 = sk_f0[e], g0 = sk_g0[e];
                    float yin;
                    yold[e] = yb;
                    if (stage == 0) {            // F0, G0 at (t0, y);  H0_1 = y + f0 h
                        sk_f0[e] = f;
                        sk_g0[e] = gfun(sk_t0[e], yb);
                        yin = yb + f * h;
                    } else if (stage == 1) {     // F1 at (t0 + h, H0_1), G1 at (t0 + h/4, H1_1);  H0_2
                        sk_f1[e] = f;
                        const float g1 = gfun(sk_t1[e], yb + 0.25f * f0 * h + SRK_B1_10 * g0 * sqh);
                        sk_g1[e] = g1;
                        const float du = sk_du[e];
                        yin = yb + 0.25f * f0 * h + 0.25f * f * h + (g0 + 0.5f * g1) * (du * (1.0f / h));      // (1 / h: one division for the tile's EPT elements)
                    } else {                     // F2 at (t0 + h/2, H0_2), G2 at (t0 + h, H1_2), G3 at (t0 + h/4, H1_3): combine
                        const float f1 = sk_f1[e], g1 = sk_g1[e], ik = sk_dw[e], ik0 = sk_du[e];
                        const float g2 = gfun(sk_t3[e], yb + f0 * h + SRK_B1_20 * g0 * sqh);
                        const float g3 = gfun(sk_t1[e], yb + 0.25f * f * h + (SRK_B1_30 * g0 + SRK_B1_31 * g1 + SRK_B1_32 * g2) * sqh);
                        const float ikk = 0.5f * (ik * ik - h);
                        const float rh = 1.0f / h, rsqh = 1.0f / sqh;      // (uniform: two divisions per pass instead of five per element)
                        const float ikkk = (ik * ik * ik - 3.0f * h * ik) * (1.0f / 6.0f);
                        const float a1 = ik, a2 = ikk * rsqh, a3 = ik0 * rh, a4 = ikkk * rh;
                        const float w0 = srk_w0(a1, a2, a3, a4);
                        const float w1 = srk_w1(a1, a2, a3, a4);
                        const float w2 = srk_w2(a1, a2, a3, a4);
                        float yn1 = yb + (f0 + f1) * (h * (1.0f / 6.0f)) + f * (h * (2.0f / 3.0f));
                        yn1 += w0 * g0 + w1 * g1 + w2 * g2 + a4 * g3;
                        sk_y[e] = yn1;
                        yin = yn1;
                    }
                    ynew[e] = yin; yv[t][e] = yin;
                    dw[t][e] = sk_dw[e];
                    continue;
                }
                float gq = gtv[t][e];
                if constexpr (CF::NN > 0) {
                    gq = gnv[FL ? 0 : e];
                }
                float q1 = 0.0f, q2 = 0.0f;
                const float raw = yfun ? snsde_phi(no, y, q1, q2) : (mul_y ? gq * y : gq);
                const float g = fast_tanh(sig_theta * snsde_nan_to_num(raw));
                float yn = fmaf(g, dw[t][e], fmaf(f, h, y));
                // Milstein: + 0.5 g dg/dy (dW^2 - h), dg/dy = (1 - g^2) sigmoid(theta) d raw/dy (raw finite)
                if (mil != 0.0f) {
                    const float draw = snsde_finite(raw) ? (yfun ? q1 : (mul_y ? gq : 0.0f)) : 0.0f;
                    yn = fmaf(mil * (g * ((1.0f - g * g) * sig_theta * draw)), fmaf(dw[t][e], dw[t][e], -h), yn);
                }
                yold[e] = y; ynew[e] = yn; yv[t][e] = yn;
            }
            const size_t goff = (size_t)row * H + fcol[t];
            if (a.act_save && row_ok) {
                float* zp = a.act_save + uoff(n, (uint32_t)nsave_rt * (uint32_t)(B * H), CF::ZSLOT, (uint32_t)(B * H)) + goff;
                if (pack_signs) {
#pragma unroll
                    for (int e = 0; e < EPT; ++e) zsave[e] = snsde_pack_signs(zsave[e], sgn >> (8 * e), snsde_save::drift_sign_bits(NHID));
                }
                if constexpr (FL) zp[0] = zsave[0];
                else *reinterpret_cast<f32x4*>(zp) = f32x4{zsave[0], zsave[1], zsave[2], zsave[3]};
            }
            sgn = 0;
            if constexpr (FL) {
                ybuf[r * LDY + fcol[t]] = ynew[0];
                if constexpr (CF::SRK) { if (a.stage_save && row_ok) a.stage_save[(size_t)(n + 1) * BH + goff] = ynew[0]; }
                if (row_ok && (!CF::SRK || stage == 2)) {
                    if (a.traj) a.traj[(size_t)(ns + 1) * BH + goff] = ynew[0];
                    if (a.dW_out) a.dW_out[(size_t)ns * BH + goff] = dw[t][0];
                    if constexpr (CF::SRK) { if (a.dU_out) a.dU_out[(size_t)ns * BH + goff] = sk_du[0]; }
                    for (int k = c_kfirst; k < c_kfirst + c_nout; ++k) {
                        const float w0 = a.out_w[2 * k], w1 = a.out_w[2 * k + 1];
                        const float o = (w0 == 0.0f) ? ynew[0] : snsde_interp_out(w0, w1, yold[0], ynew[0]);
                        if (!a.row_out) a.ys[(size_t)(k + 1) * BH + goff] = o;
                        else if (rslot == k + 1) a.ys[goff] = o;
                    }
                }
            } else {
                const f32x4 vn = {ynew[0], ynew[1], ynew[2], ynew[3]};
                *reinterpret_cast<f32x4*>(ybuf + r * LDY + fcol[t]) = vn;
                if constexpr (CF::SRK) { if (a.stage_save && row_ok) *reinterpret_cast<f32x4*>(a.stage_save + (size_t)(n + 1) * BH + goff) = vn; }
                if (row_ok && (!CF::SRK || stage == 2)) {
                    if (a.traj) *reinterpret_cast<f32x4*>(a.traj + (size_t)(ns + 1) * BH + goff) = vn;
                    if (a.dW_out) *reinterpret_cast<f32x4*>(a.dW_out + (size_t)ns * BH + goff) =
                        f32x4{dw[t][0], dw[t][1], dw[t][2], dw[t][3]};
                    if constexpr (CF::SRK) {
                        if (a.dU_out) *reinterpret_cast<f32x4*>(a.dU_out + (size_t)ns * BH + goff) =
                            f32x4{sk_du[0], sk_du[EPT > 1 ? 1 : 0], sk_du[EPT > 2 ? 2 : 0], sk_du[EPT > 3 ? 3 : 0]};
                    }
                    for (int k = c_kfirst; k < c_kfirst + c_nout; ++k) {
                        const float w0 = a.out_w[2 * k], w1 = a.out_w[2 * k + 1];
                        f32x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (w0 == 0.0f) ? ynew[e] : snsde_interp_out(w0, w1, yold[e], ynew[e]);
                        if (!a.row_out) *reinterpret_cast<f32x4*>(a.ys + (size_t)(k + 1) * BH + goff) = o;
                        else if (rslot == k + 1) *reinterpret_cast<f32x4*>(a.ys + goff) = o;
                    }
                }
            }
        }
        TRACE(8)
        __syncthreads();
        TRACE(9)
    }
#ifdef SNSDE_TRACE
    if (blockIdx.x == 0 && lane == 0 && a.dW_out) {
        for (int i = 0; i < 10; ++i) a.dW_out[wave * 16 + i] = (float)tr_acc[i];
    }
#endif
}

template <class CF>
int launch_cfg(const MfmaArgs& a, hipStream_t stream) {
    const size_t lds_bytes = (size_t)(a.dW ? CF::LDS_BASE : CF::LDS_FLOATS) * sizeof(float);
    static SnsdeLdsAttr lds_attr;   // per instantiation and device
    if (const int rc = snsde_lds_attr(reinterpret_cast<const void*>(snsde_mfma_kernel<CF>), lds_bytes, lds_attr)) return rc;
    const int members = a.members > 1 ? a.members : 1;      // (model ensembles: tiles of a member x members; one model: a grid of one row)
    const int grid = ((members > 1 ? a.member_rows : a.B) + CF::M - 1) / CF::M;
    hipLaunchKernelGGL(snsde_mfma_kernel<CF>, dim3(grid, members), dim3(CF::NT), lds_bytes, stream, a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

// =====================================================================================================
// Backward: adjoint recursion of the Euler scheme over the saved trajectory (include/snsde.h, snsde_backward).
// Same skeleton as the forward kernel (persistent row tiles, one 16-feature tile per wave, register-stationary
// weights, transposed f32 MFMA chain), run on the TRANSPOSED matrices:
//     dzout -> out^T -> [z_hid > 0] -> hid^T .. -> [z0 > 0] -> first_y^T -> dy
// where first_y = (emb o linear_in)[:, y columns] (or linear_in[:, y columns] without emb).  relu masks and the
// pre-tanh drift come from the forward's act_save; f, g and their derivatives are recomputed elementwise.
// =====================================================================================================
template <int H_, int NHID_, int GEO_, int FL_, int NN_ = 0, int IO0_ = 0>
struct CfgR {
    static constexpr int H = H_, NHID = NHID_, FL = FL_, NN = NN_;
    static constexpr bool IO0 = IO0_ != 0;       // y-free drift (input_option 0): its chain ends at the first layer's delta   // NN: layers of the diffusion net on [tau, y] (noise_option 14/15: 1, 18/19: 2)
    static constexpr bool GEO = GEO_ != 0;
    static constexpr int TPW = 1;
    static constexpr int NW = H / 16;
    static constexpr int NT = NW * 64;
    static constexpr int WPS = NW >= 4 ? NW / 4 : 1;
    static constexpr int M = FL ? 4 : 16;
    static constexpr int KUH = H / 16;
    static constexpr int PAD = FL ? 16 : 8;
    static constexpr int LDA = ld_for(16 * KUH, PAD);
    static constexpr int ND = NHID + (IO0 ? 1 : 2);   // transposed GEMMs of the drift chain
    static constexpr int NG = ND + NN;           // + the diffusion net's
    static constexpr int NBUF = snsde_save::delta_slots(NHID, NN, SNSDE_EULER);   // LDS buffers = delta slots (snsde_save_layout.h)
    static constexpr int NSAVE = snsde_save::act_slots(NHID, NN, SNSDE_EULER);
    static constexpr int ZSLOT = snsde_save::act_z(NHID);
    static constexpr int EPT = FL ? 1 : 4;
    static constexpr int ROWCH = 128;
    static constexpr bool STREAM = H > 128;
    static constexpr bool RING = STREAM && FL;   // transposed weights through the per-wave LDS ring (as snsde_m4s_kernel.h)
    static constexpr int ACC0 = NBUF * M * LDA + (ROWCH + 1) * SNSDE_STEP_STRIDE;         // 16 floats: the accumulator column's cotangent per tile row
    static constexpr int RING0 = ACC0 + 16;                                                // multiple of 4 floats
    static constexpr int LDS_FLOATS = RING0 + (RING ? NW * 8 * 256 : 0);
};

struct RevArgs {
    const float* params;
    const float* ws;        // backward workspace: packed transposed weights
    const float* gt;        // time-only diffusion table (N, H) of the forward workspace, or null
    const float* step_tab;
    const float* out_w;
    const float* traj;
    const float* act;
    const float* dW;
    const float* dU;   // SRK: the space-time Levy integrals used by the forward
    const float* grad_ys;
    float* adj;
    float* delta;      // (N, NG, B, H) or null
    const int32_t* row_out;   // (B) per-row output slot (grad_ys is then (B, H)) or null
    float* ds_part;    // (workgroups, N, H) per-tile sums of dL/d s_n (time-only diffusion table), or null
    float* dth_part;   // (workgroups, waves) partial sums of dL/d sigmoid(theta), or null
    int32_t B, N, T, no, off_theta, method;
    int32_t w_off[MAXL];
    int32_t nsave;                     // activation slots per step in `act` (snsde_act_slots)
    int32_t act_fn, f_out, g_out;      // field variants (SNSDE_ACT_*, SNSDE_DRIFT_*, SNSDE_DIFFUSION_*): 4-row tiles only
    int32_t geo;                       // snsde_m4n_rev_kernel.h: the drift is gated by tanh(y) (input_option 5 / 6)
    int32_t adj0_only;                 // SNSDE_BWD_ADJ0_ONLY: `adj` is (B, H) = dL/dy0; the intermediate adjoints are not written
    // dW == null: the forward drew its increments from Philox with this key / row offset and did not write them out; the
    // Euler / Milstein adjoint regenerates them (same call, same product z * sqrt h: bit-identical)
    uint64_t seed;
    int64_t row_offset;
    int32_t step_offset;               // n0 of a continued solve: local step n regenerates the normals of global step n0 + n (uniform)
    int32_t acc_col;                   // path-integral accumulator column (-1: none) and its prior drift a y + b
    float acc_a, acc_b;
    // model ensembles under SNSDE_FLAG_ENSEMBLE_GRAD (snsde_solve::members = M > 1): the member is the second grid axis of the general
    // adjoint's launches, m = blockIdx.y (one model: a grid of one row, m = 0, member_rows and the strides 0), as in the forward
    // (MfmaArgs) - tile blockIdx.x of member m covers rows m member_rows + 4 blockIdx.x .. of the (.., B, H) planes and reads
    // params + m param_stride, ws + m ws_stride (packed transposed weights; ds_part / dth_part lie in the same block: the member's own
    // nwg = member_rows / 4 partial blocks, indexed by blockIdx.x as in the member's own solve) and gt + m gt_stride (the table inside
    // block m of the forward workspace); M ws_stride and M gt_stride fit 32 bits (snsde_mfma_backward_launch).  Read by snsde_mfma_reverse_kernel and snsde_mfma_srk_reverse_kernel only.
    int32_t members, member_rows;
    uint32_t param_stride, ws_stride, gt_stride;
};

// float offset of member blockIdx.y's block of the backward workspace (RevArgs::ws_stride; one model: 0).  Formed where it is used
// and not held in a variable across the step loop: the adjoint kernels run at their scalar-register limit, and a value kept live
// through the loop cost the y-free and the deepest SRK instantiations a spilled scalar register each (one of them a wave per SIMD)
__device__ __forceinline__ uint32_t rev_member_ws(const RevArgs& a) { return blockIdx.y * a.ws_stride; }

// d/dx [scale * x * sigmoid(x)]  (LipSwish: scale = 0.909, SiLU: 1)
__device__ __forceinline__ float swish_grad(float x, float scale) {
    const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
    return scale * sg * fmaf(x, 1.0f - sg, 1.0f);
}

template <class CF>
__global__ void __launch_bounds__(CF::NT, CF::WPS) snsde_mfma_reverse_kernel(RevArgs a) {
    constexpr int H = CF::H, TPW = 1, FL = CF::FL, M = CF::M, NT = CF::NT, NHID = CF::NHID, NG = CF::NG;
    constexpr int NS = CF::NBUF;                 // LDS buffers = delta slots: z_out, hidden.., first layer, [diffusion net]
    constexpr int NB0 = snsde_save::delta_net(NHID, 0);      // first buffer / slot of the diffusion net's chain
    constexpr bool IO0 = CF::IO0;
    constexpr int NM = IO0 ? CF::ND : CF::ND - 1;   // relu masks of the drift chain
    constexpr int KUH = CF::KUH, EPT = CF::EPT, LDA = CF::LDA, ND = CF::ND, NN = CF::NN;
    const int NSAVE = a.nsave;                   // activation slots per step (the smooth-activation variants save more)
    const bool variant = FL && (a.act_fn != 0 || a.f_out != 0 || a.g_out != 0);      // tutorial-style fields (4-row tiles)
    const float act_scale = a.act_fn == SNSDE_ACT_LIPSWISH ? 0.909f : 1.0f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* rowtab = lds + NS * M * LDA;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = FL ? (lane & 3) : (lane & 15);
    const int s = FL ? ((lane >> 2) & 3) : (lane >> 4);
    const int fsub = FL ? 4 * (lane >> 4) : 4 * s;
    // model ensembles: blockIdx.y is the member (RevArgs::members; one model: 0) - its first row and its blocks, formed once
    // (32-bit uniform offsets formed where they are used, not rebased pointers held across the step loop: the kernarg values stay
    //  re-loadable - the launcher checks that M blocks fit 32 bits)
    const int row0 = (int)blockIdx.y * a.member_rows + blockIdx.x * M, B = a.B;
    const int row = row0 + r, rowc = row < B ? row : B - 1;
    const bool row_ok = row < B;
    const size_t BH = (size_t)B * H;
    const bool writer = FL ? (s == 0) : true;
    const bool s1 = (s == 1), s2 = (s == 2), s3 = (s == 3);
    const int fcol = wave * 16 + fsub + (FL ? s : 0);
    const uint32_t goff = (uint32_t)(rowc * H + fcol);     // (32-bit lane offset: loads take the scalar-base form)

    Wt<CF::STREAM, KUH, TPW> wt[NG];
    uint64_t sbr[NG];                 // RING: this wave's slice of every transposed matrix (SGPR pairs)
    uint32_t ring_m0 = 0, ring_ra = 0, ring_lo = 0, ring_hi = 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if constexpr (CF::RING) sbr[g] = lean_uniform(a.ws + rev_member_ws(a) + a.w_off[g] + (size_t)wave * KUH * 256);
        else wt[g].load(a.ws + rev_member_ws(a) + a.w_off[g], wave, lane);
    }
    if constexpr (CF::RING) {
        const uint32_t ringb = lean_lds_addr(lds + CF::RING0) + (uint32_t)wave * (8 * 1024);
        ring_m0 = __builtin_amdgcn_readfirstlane(ringb + 4096u);
        ring_ra = ringb + (uint32_t)lane * 16u;
        ring_lo = (uint32_t)lane * 16u + 4096u;
        ring_hi = ring_lo + 8192u;
        // the ring's first eight blocks (GEMM 0); every later block is requested eight blocks ahead of its use
        stream_refill<0>(ring_m0, ring_lo, ring_hi, sbr[0]); stream_refill<1>(ring_m0, ring_lo, ring_hi, sbr[0]);
        stream_refill<2>(ring_m0, ring_lo, ring_hi, sbr[0]); stream_refill<3>(ring_m0, ring_lo, ring_hi, sbr[0]);
        stream_refill<4>(ring_m0, ring_lo, ring_hi, sbr[0]); stream_refill<5>(ring_m0, ring_lo, ring_hi, sbr[0]);
        stream_refill<6>(ring_m0, ring_lo, ring_hi, sbr[0]); stream_refill<7>(ring_m0, ring_lo, ring_hi, sbr[0]);
    }
    for (int i = tid; i < NS * M * LDA; i += NT) lds[i] = 0.0f;

    const float sig_theta = snsde_sigmoid((a.params + (size_t)blockIdx.y * a.param_stride)[a.off_theta]);
    const bool mul_y = (a.no == 13 || a.no == 17 || a.no == 15 || a.no == 19 || a.no == 3 || a.no == 6 || a.no == 11);
    const bool yfun = (a.no >= 7 && a.no <= 10);     // raw = phi(y): no table, theta is the only diffusion parameter
    const float mil = (a.method == SNSDE_MILSTEIN) ? 0.5f : 0.0f;

    auto fill_rows = [&](int base) {
        for (int i = tid; i < (CF::ROWCH + 1) * SNSDE_STEP_STRIDE; i += NT) {
            const int rr = base + i / SNSDE_STEP_STRIDE;
            rowtab[i] = a.step_tab[(size_t)(rr < a.N ? rr : a.N - 1) * SNSDE_STEP_STRIDE + i % SNSDE_STEP_STRIDE];
        }
    };

    // adjoint of y_N (owned elements)
    float adj[EPT], gfin[EPT];
    const int rslot = a.row_out ? a.row_out[rowc] : -1;     // per-row output selection: the row's single output gradient
#pragma unroll
    for (int e = 0; e < EPT; ++e) { adj[e] = 0.0f; gfin[e] = a.row_out ? a.grad_ys[goff + e] : 0.0f; }
    int rbase = -1;
    const bool dsum = a.ds_part != nullptr && a.gt != nullptr;   // diffusion-side parameter sums wanted (time-only noise MLP)
    const float rowf = row_ok ? 1.0f : 0.0f;                     // padding rows replicate the last row: excluded
    float th_acc = 0.0f;

    // per-step inputs from HBM are fetched one step ahead, so their latency hides behind the previous step's GEMM chain
    // M16: the writer lanes hold the relu masks of their four features (f32x4); M4: after the k-slot reduce-scatter every
    // lane owns ONE output (row r, feature fcol).  Relu: the drift chain's masks are bits of z (snsde_pack_signs); `mask` holds the
    // pre-activations of the smooth-activation variants (4-row tiles only), `nmask` the hidden activation of a two-layer diffusion net.
    struct StepIn { f32x4 nmask; float mask[4]; float y[EPT], z[EPT], dw[EPT], gq[EPT]; };
    static_assert(NM <= 4, "mask slots");
    // cur <-> nxt move member by member, and only the members this flavour uses: a whole-struct assignment also copies the members a
    // flavour never touches, and those bytes travel through scratch memory every step (16 bytes of nmask each way before round 4; 48
    // when the 16-row-tile kernel's mask planes went away: 1437 -> 1867 us at K3 until this was found)
    auto step_copy = [&](StepIn& d, const StepIn& sfrom) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) { d.y[e] = sfrom.y[e]; d.z[e] = sfrom.z[e]; d.dw[e] = sfrom.dw[e]; d.gq[e] = sfrom.gq[e]; }
        if constexpr (FL) {
#pragma unroll
            for (int g = 0; g < NM; ++g) d.mask[g] = sfrom.mask[g];
        }
        if constexpr (NN == 2) d.nmask = sfrom.nmask;
    };
    float zblk[EPT][4];                 // regenerated increments: the normals of the 4-step block being walked
    int zblk_id = -1;
    const uint32_t grow = (uint32_t)(a.row_offset + row);
    const uint32_t BH32 = (uint32_t)BH, SBH = (uint32_t)NSAVE * BH32, NSBH = (uint32_t)NS * BH32;     // uniform strides (see uoff)
    const uint32_t pre0 = a.act_fn != 0 ? (uint32_t)snsde_save::act_pre(NHID, NN, SNSDE_EULER, 0) : 0u;      // smooth activations: first PRE-activation slot
    auto prefetch = [&](int n, StepIn& p) {
        if (!a.dW) {                    // (wave-uniform)
            const int gn = a.step_offset + n;      // the global step: its block is cached while the walk stays inside it
            if ((gn >> 2) != zblk_id) {
                zblk_id = gn >> 2;
#pragma unroll
                for (int e = 0; e < EPT; ++e) snsde_philox_normal4(a.seed, grow, (uint32_t)zblk_id, (uint32_t)(fcol + e), zblk[e]);
            }
            const float sqh = a.step_tab[uoff(n, SNSDE_STEP_STRIDE) + 6];
            const int k = gn & 3;
#pragma unroll
            for (int e = 0; e < EPT; ++e)
                p.dw[e] = (k == 0 ? zblk[e][0] : (k == 1 ? zblk[e][1] : (k == 2 ? zblk[e][2] : zblk[e][3]))) * sqh;
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            p.y[e] = (a.traj + uoff(n, BH32))[goff + e];
            p.z[e] = (a.act + uoff(n, SBH, CF::ZSLOT, BH32))[goff + e];
            if (a.dW) p.dw[e] = (a.dW + uoff(n, BH32))[goff + e];
            if constexpr (NN > 0) p.gq[e] = (a.act + uoff(n, SBH, snsde_save::act_net_out(NHID, NN), BH32))[goff + e];   // diffusion-net output
            else p.gq[e] = a.gt ? (a.gt + uoff(n, H, blockIdx.y, a.gt_stride))[fcol + e] : 0.0f;      // (row n of the member's table)
        }
        if constexpr (FL) {
            if (__builtin_expect(a.act_fn != 0, 0)) {      // relu: the signs ride in z's low bits (snsde_pack_signs)
#pragma unroll
            for (int g = 0; g < NM; ++g)     // smooth activations: the PRE-activation of the forward activation feeding transposed GEMM g + 1 (slots behind the net's)
                p.mask[g] = (a.act + uoff(n, SBH, (uint32_t)(NHID - g) + pre0, BH32))[goff];
            }
            if constexpr (NN == 2)               // hidden activation of the diffusion net (smooth: its pre-activation, the last slot)
                p.nmask[0] = (a.act + uoff(n, SBH, a.act_fn != 0 ? (uint32_t)NSAVE - 1u : (uint32_t)snsde_save::act_net(NHID, 0), BH32))[goff];
        } else if (writer) {      // (16-row tiles: relu only - the drift chain's masks come out of z)
            if constexpr (NN == 2)
                p.nmask = *reinterpret_cast<const f32x4*>(
                    a.act + uoff(n, SBH, snsde_save::act_net(NHID, 0), BH32) + (uint32_t)(rowc * H + wave * 16 + fsub));
        }
    };
    constexpr bool AHEAD = !CF::STREAM || CF::RING;   // (the M16 streamed-weight variant has no registers to spare for it)
    StepIn cur, nxt;
    if constexpr (AHEAD) prefetch(a.N - 1, cur);

    for (int n = a.N - 1; n >= 0; --n) {
        if constexpr (AHEAD) {
            step_copy(nxt, cur);
            if (n > 0) prefetch(n - 1, nxt);
        } else {
            prefetch(n, cur);
        }
        const int nb = (n / CF::ROWCH) * CF::ROWCH;
        if (nb != rbase) {           // (re)stage the step-table chunk; previous step's readers are past its last barrier
            __syncthreads();
            rbase = nb;
            fill_rows(rbase);
            __syncthreads();
        }
        const float* st = rowtab + (n - rbase) * SNSDE_STEP_STRIDE;
        const float h = st[1];
        const int nout = __float_as_int(st[8]), kfirst = __float_as_int(st[9]);

        // outputs emitted after step n: ys[k+1] = y_{n+1}  or  w0 y_n + w1 y_{n+1}
        float carry[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) carry[e] = 0.0f;
        for (int k = kfirst; k < kfirst + nout; ++k) {
            const float w0 = a.out_w[2 * k], w1 = a.out_w[2 * k + 1];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const float gk = a.row_out ? (rslot == k + 1 ? gfin[e] : 0.0f) : (a.grad_ys + uoff(k + 1, BH32))[goff + e];
                if (w0 == 0.0f) adj[e] += gk;
                else { adj[e] = fmaf(w1, gk, adj[e]); carry[e] = fmaf(w0, gk, carry[e]); }
            }
        }
        if (row_ok && !a.adj0_only) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) (a.adj + uoff(n + 1, BH32))[goff + e] = adj[e];
        }
        // path-integral accumulator column (snsde.h: kl_column1): its state adjoint x h is the cotangent of the KL rate u of this step;
        // the owner lane publishes it to the tile row (one more barrier per step), every latent lane adds d u / d f_j and d u / d y_j
        float fbA = 0.0f;
        if constexpr (FL) {
            if (__builtin_expect(a.acc_col >= 0, 0)) {
                float* accb = lds + CF::ACC0;
                if ((int)fcol == a.acc_col) accb[r] = adj[0] * h;
                __syncthreads();
                fbA = accb[r];
            }
        }
        // ---- elementwise: d(f h + g dW)/d(zout, y) applied to the adjoint ----
        float ay[EPT], dz[EPT], dsv[EPT], dq[EPT];
        const uint32_t zclear = a.act_fn == 0 ? ~((1u << snsde_save::drift_sign_bits(NHID)) - 1u) : ~0u;
        uint32_t zb[EPT];      // bit pattern of the saved z: its low NHID + 1 bits are the relu signs of the step (snsde_pack_signs)
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            dsv[e] = 0.0f; dq[e] = 0.0f;
            zb[e] = __builtin_bit_cast(uint32_t, cur.z[e]);
            // (the sign bits are cleared before z is used: an infinite z of a diverged solve stays infinite instead of becoming a NaN)
            const float y = cur.y[e], z = __builtin_bit_cast(float, zb[e] & zclear), dw = cur.dw[e], gq = cur.gq[e];
            const float av = adj[e];
            if (__builtin_expect(variant, 0)) {
                // f = tanh z | z | z y;  g = raw = s_n or s_n y (SNSDE_DIFFUSION_RAW), else the reference's tanh(sigmoid(theta) raw)
                float fz = 1.0f, acc = av;
                if (a.f_out == SNSDE_DRIFT_TANH) { const float f = fast_tanh(z); fz = 1.0f - f * f; }
                else if (a.f_out == SNSDE_DRIFT_TIMES_Y) { fz = y; acc = fmaf(av * h, z, acc); }
                dz[e] = av * h * fz;
                if (FL && __builtin_expect(a.acc_col >= 0, 0)) {      // (linear drift output: f = z)
                    if ((int)fcol < a.acc_col) {
                        const float inv = snsde_stable_inv(gq);
                        const float ue = (z - fmaf(a.acc_a, y, a.acc_b)) * inv * inv * fbA;      // fbA d u / d f_j
                        dz[e] += ue;
                        acc = fmaf(-a.acc_a, ue, acc);                                           // fbA d u / d y_j
                    } else if ((int)fcol == a.acc_col) {
                        dz[e] = 0.0f;                                  // the owner's drift is u, not the net's output
                    }
                }
                const float qq = mil * fmaf(dw, dw, -h);
                float d = 0.0f;
                if constexpr (NN > 0) {
                    // NeuralSDEFunc-shaped fields (Euler): g = raw = q {y}, q the net's output (linear for SNSDE_DIFFUSION_RAW_NET,
                    // rectified for SNSDE_DIFFUSION_RAW); the cotangent of q enters the net's transposed chain
                    float dqv = mul_y ? av * dw * y : av * dw;
                    if (mul_y) acc = fmaf(av * dw, gq, acc);
                    if (NN == 2 && a.g_out != SNSDE_DIFFUSION_RAW_NET) dqv = gq > 0.0f ? dqv : 0.0f;
                    dq[e] = dqv;
                } else
                if (a.g_out == SNSDE_DIFFUSION_RAW) {
                    if (mul_y) { acc = fmaf(av * gq, fmaf(qq, gq, dw), acc); d = av * rowf * y * fmaf(2.0f * qq, gq, dw); }
                    else d = av * rowf * dw;
                } else {
                    const float raw = mul_y ? gq * y : gq;
                    const float g = fast_tanh(sig_theta * snsde_nan_to_num(raw));
                    const float om = 1.0f - g * g;
                    const bool finite = snsde_finite(raw);
                    if (mul_y && finite) {
                        const float c = sig_theta * gq;
                        acc = fmaf(av * om * c, dw + qq * c * fmaf(-3.0f * g, g, 1.0f), acc);
                    }
                    const float du = av * dw * om * rowf;
                    d = finite ? du * sig_theta * (mul_y ? y : 1.0f) : 0.0f;
                    if (mul_y && finite && mil != 0.0f)
                        d = fmaf(av * rowf * om * qq * fmaf(fmaf(-3.0f * g, g, 1.0f) * sig_theta * gq, y, g), sig_theta, d);
                }
                ay[e] = acc;
                if (dsum) dsv[e] = d;
                continue;
            }
            float ty = 1.0f, zt = z;
            if constexpr (CF::GEO) { ty = fast_tanh(y); zt = z * ty; }
            const float f = fast_tanh(zt);
            const float dzt = av * h * (1.0f - f * f);
            float acc_y = av;
            if constexpr (CF::GEO) { dz[e] = dzt * ty; acc_y = fmaf(dzt * z, 1.0f - ty * ty, acc_y); }
            else dz[e] = dzt;
            float q1 = 0.0f, q2 = 0.0f;
            const float raw = yfun ? snsde_phi(a.no, y, q1, q2) : (mul_y ? gq * y : gq);
            const float rcv = snsde_nan_to_num(raw);
            const float g = fast_tanh(sig_theta * rcv);
            const bool finite = snsde_finite(raw);
            const float om = 1.0f - g * g;
            if (yfun) {
                if (finite) {
                    // g' = (1 - g^2) s r1,  g'' = (1 - g^2) s r2 - 2 g g' s r1  (s = sigmoid(theta));  d/dy [g dW + mil (dW^2 - h) g g']
                    const float g1 = om * sig_theta * q1;
                    const float g2 = om * sig_theta * q2 - 2.0f * g * g1 * sig_theta * q1;
                    const float qq = mil * fmaf(dw, dw, -h);
                    acc_y = fmaf(av, fmaf(qq, fmaf(g1, g1, g * g2), dw * g1), acc_y);
                    // d/d sigmoid(theta): (1 - g^2) rc dW + mil (dW^2 - h)(1 - g^2) r1 [s rc (1 - 3 g^2) + g]
                    th_acc = fmaf(av * rowf * om, fmaf(qq * q1, fmaf(sig_theta * rcv, fmaf(-3.0f * g, g, 1.0f), g), dw * rcv), th_acc);
                } else {
                    th_acc = fmaf(av * rowf * om * dw, rcv, th_acc);
                }
            } else if (mul_y && finite) {
                // d/dy [g dW + mil (dW^2 - h) g g'],  g' = (1 - g^2) c,  (g g')' = c^2 (1 - g^2)(1 - 3 g^2),  c = sigmoid(theta) s_n
                const float c = sig_theta * gq;
                const float dm = mil * fmaf(dw, dw, -h) * c * fmaf(-3.0f * g, g, 1.0f);
                acc_y = fmaf(av * om * c, dw + dm, acc_y);
            }
            if constexpr (NN > 0) {
                // raw = q (14, 18) or q * y (15, 19), q = the diffusion net's output (relu'd for 18/19): Euler term g dW
                const float dr = finite ? av * dw * om * sig_theta : 0.0f;
                float d = mul_y ? dr * y : dr;
                if constexpr (NN == 2) d = gq > 0.0f ? d : 0.0f;
                dq[e] = d;
                th_acc = fmaf(av * dw * om * rowf, rcv, th_acc);
            }
            ay[e] = acc_y;
            if (dsum) {
                // parameter side of the same term:  d/d sigmoid(theta) and d/d s_n of  g dW + mil (dW^2 - h) g g'
                const float du = av * dw * om * rowf;
                th_acc = fmaf(du, rcv, th_acc);
                float d = finite ? du * sig_theta * (mul_y ? y : 1.0f) : 0.0f;
                if (mul_y && finite && mil != 0.0f) {
                    const float c = sig_theta * gq;
                    const float ex = av * rowf * om * (mil * fmaf(dw, dw, -h)) * fmaf(fmaf(-3.0f * g, g, 1.0f) * c, y, g);
                    th_acc = fmaf(ex, gq, th_acc);
                    d = fmaf(ex, sig_theta, d);
                }
                dsv[e] = d;
            }
        }
        if (dsum) {     // sum over the tile's rows, one writer lane per feature
            float* dp = a.ds_part + rev_member_ws(a) + ((size_t)blockIdx.x * a.N + n) * H + fcol;
            if constexpr (FL) {     // rows = lane & 3
                float v = dsv[0];
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));
                if (r == 0) dp[0] = v;
            } else {                // rows = lane & 15
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    float v = dsv[e];
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));
                    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
                    dsv[e] = v;
                }
                if (r == 0) *reinterpret_cast<f32x4*>(dp) = f32x4{dsv[0], dsv[1], dsv[2], dsv[3]};
            }
        }
        float* buf = lds;   // buffer g holds the input of transposed GEMM g
        if constexpr (FL) buf[r * LDA + fcol] = dz[0];
        else *reinterpret_cast<f32x4*>(buf + r * LDA + fcol) = f32x4{dz[0], dz[1], dz[2], dz[3]};
        if (a.delta && row_ok) {
            float* dp = a.delta + uoff(n, NSBH) + goff;
            if constexpr (FL) dp[0] = dz[0];
            else *reinterpret_cast<f32x4*>(dp) = f32x4{dz[0], dz[1], dz[2], dz[3]};
        }
        if constexpr (NN > 0) {     // input of the diffusion net's transposed chain (buffer / delta slot NB0)
            float* nb = lds + NB0 * M * LDA;
            if constexpr (FL) nb[r * LDA + fcol] = dq[0];
            else *reinterpret_cast<f32x4*>(nb + r * LDA + fcol) = f32x4{dq[0], dq[1], dq[2], dq[3]};
            if (a.delta && row_ok) {
                float* dp = a.delta + uoff(n, NSBH, NB0, BH32) + goff;
                if constexpr (FL) dp[0] = dq[0];
                else *reinterpret_cast<f32x4*>(dp) = f32x4{dq[0], dq[1], dq[2], dq[3]};
            }
        }
        if constexpr (IO0) {        // the drift does not see y: its chain only produces the layer deltas
#pragma unroll
            for (int e = 0; e < EPT; ++e) adj[e] = ay[e] + carry[e];
        }
        __syncthreads();
        f32x4 acc[TPW], acc2[TPW];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int bi = g < ND ? g : NB0 + (g - ND);     // LDS buffer / delta slot holding this GEMM's input
            const bool mid = (g < ND - 1) || (g == ND - 1 && IO0) || (g >= ND && g != NG - 1);
            acc[0] = acc2[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (CF::RING)
                stream_layer<0>(lean_lds_addr(lds + bi * M * LDA + r * LDA + 4 * s), ring_ra, ring_m0, ring_lo, ring_hi, sbr[g],
                                sbr[(g + 1) % NG], acc[0], acc2[0]);
            else
                gemm<FL, KUH, TPW>(wt[g], lds + bi * M * LDA + r * LDA + 4 * s, acc, acc2);
            f32x4 v = acc[0] + acc2[0];
            if constexpr (FL) {
                // k-slot reduce-scatter (6 DPP ops): this lane's single output (row r, feature fcol)
                const float o = m4_reduce_scatter(v);
                if (mid) {
                    const float zs = g < ND ? cur.mask[g < NM ? g : 0] : cur.nmask[0];
                    float dv;
                    if (__builtin_expect(a.act_fn != 0, 0)) dv = o * swish_grad(zs, act_scale);
                    else if (g < ND) dv = ((zb[0] >> (NHID - g)) & 1u) ? o : 0.0f;      // sign of act slot NHID - g
                    else dv = zs > 0.0f ? o : 0.0f;
                    lds[(bi + 1) * M * LDA + r * LDA + fcol] = dv;
                    if (a.delta && row_ok) (a.delta + uoff(n, NSBH, bi + 1, BH32))[goff] = dv;
                    __syncthreads();
                } else if (g == ND - 1) {
                    adj[0] = ay[0] + o + carry[0];      // end of the drift chain
                } else {
                    adj[0] += o;                        // end of the diffusion net's chain
                }
                continue;
            }
            if (mid) {
                // relu mask of the forward activation that produced this gradient's input: slot NHID - g (drift chain),
                // the diffusion net's hidden activation (first GEMM of its chain, noise_option 18/19)
                if (writer) {
                    if (g < ND) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = ((zb[i < EPT ? i : 0] >> (NHID - g)) & 1u) ? v[i] : 0.0f;
                    } else {
                        const f32x4 zsv = cur.nmask;
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = zsv[i] > 0.0f ? v[i] : 0.0f;
                    }
                    *reinterpret_cast<f32x4*>(lds + (bi + 1) * M * LDA + r * LDA + wave * 16 + fsub) = v;
                    if (a.delta && row_ok)
                        *reinterpret_cast<f32x4*>(a.delta + uoff(n, NSBH, bi + 1, BH32) + (uint32_t)(row * H + wave * 16 + fsub)) = v;
                }
                __syncthreads();
            } else {
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    float d = v[FL ? 0 : e];
                    if constexpr (FL) { d = s1 ? v[1] : d; d = s2 ? v[2] : d; d = s3 ? v[3] : d; }
                    if (g == ND - 1) adj[e] = ay[e] + d + carry[e];      // end of the drift chain
                    else adj[e] += d;                                    // end of the diffusion net's chain
                }
            }
        }
        if constexpr (AHEAD) step_copy(cur, nxt);
    }
    if (row_ok) {     // ys[0] = y0
#pragma unroll
        for (int e = 0; e < EPT; ++e) a.adj[goff + e] = adj[e] + (a.row_out ? (rslot == 0 ? gfin[e] : 0.0f) : a.grad_ys[goff + e]);
    }
    if ((dsum || NN > 0 || yfun) && a.dth_part) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) th_acc += __shfl_down(th_acc, off, 64);
        if (lane == 0) (a.dth_part + rev_member_ws(a))[blockIdx.x * CF::NW + wave] = th_acc;
    }
    if constexpr (CF::RING) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the ring's last requests land before the wave ends
}

template <class CF>
int launch_rev(const RevArgs& a, hipStream_t stream) {
    const size_t lds_bytes = (size_t)CF::LDS_FLOATS * sizeof(float);
    static SnsdeLdsAttr lds_attr;   // per instantiation and device
    if (const int rc = snsde_lds_attr(reinterpret_cast<const void*>(snsde_mfma_reverse_kernel<CF>), lds_bytes, lds_attr)) return rc;
    const int members = a.members > 1 ? a.members : 1;      // (model ensembles: tiles of a member x members; one model: a grid of one row)
    if (members > 1 && !CF::FL) return SNSDE_ERR_UNSUPPORTED;      // (a 16-row tile would straddle members: route_backward plans 4-row tiles)
    const int grid = ((members > 1 ? a.member_rows : a.B) + CF::M - 1) / CF::M;
    hipLaunchKernelGGL(snsde_mfma_reverse_kernel<CF>, dim3(grid, members), dim3(CF::NT), lds_bytes, stream, a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}


// =====================================================================================================
// SRK (SRID2) adjoint on the MFMA path, M4 tiles.  The forward ran every solver step as three drift passes and saved,
// per pass p = 3n + s, the layer activations (act_save[p]) — so the backward of a step is three transposed chains
// (stage 2, 1, 0: same register-stationary chain as the Euler adjoint, relu masks and deltas indexed by pass) glued by
// the elementwise reverse of the stage combinations:
//     Fbar_s, Gbar_s <- a (alpha_s h, w_s) + the H0/H1 combinations of later stages,
//     H1bar_s = Gbar_s dg/dy(t1_s, H1_s),   H0bar_s = J_f^T Fbar_s (the chain).
// F_s, G_s, H0_s, H1_s are recomputed per lane from y_n, the saved pre-tanh drifts and (I_k, I_k0).  The diffusion-side
// parameter sums (d/d sigmoid(theta), d/d s(t) at the stage times: rows 4n + slot) are left per workgroup as in the
// Euler adjoint.
// =====================================================================================================
template <class CF>
__global__ void __launch_bounds__(CF::NT, CF::WPS) snsde_mfma_srk_reverse_kernel(RevArgs a) {
    static_assert(CF::FL == 1 && CF::NN == 0, "SRK adjoint: M4 tiles, elementwise diffusions");
    constexpr int H = CF::H, TPW = 1, M = CF::M, NT = CF::NT, NHID = CF::NHID, NG = CF::NG;
    constexpr int KUH = CF::KUH, LDA = CF::LDA;
    const int NSAVE = a.nsave;                   // activation slots per pass (the smooth-activation variants save more)
    const uint32_t SBH = (uint32_t)NSAVE * (uint32_t)(a.B * H), NGBH = (uint32_t)NG * (uint32_t)(a.B * H);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 3, s = (lane >> 2) & 3, fsub = 4 * (lane >> 4);
    // model ensembles: blockIdx.y is the member (RevArgs::members; one model: 0) - its first row and its blocks, formed once
    const int row0 = (int)blockIdx.y * a.member_rows + blockIdx.x * M, B = a.B;      // (offsets: rev_member_ws, as in the Euler adjoint)
    const int row = row0 + r, rowc = row < B ? row : B - 1;
    const bool row_ok = row < B;
    const size_t BH = (size_t)B * H;
    const bool writer = (s == 0);
    const bool s1 = (s == 1), s2 = (s == 2), s3 = (s == 3);
    const int fcol = wave * 16 + fsub + s;
    const uint32_t goff = (uint32_t)(rowc * H + fcol);
    const uint32_t BH32 = (uint32_t)BH;                 // uniform strides as 32-bit factors (uoff: scalar-unit products)

    Wt<CF::STREAM, KUH, TPW> wt[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) wt[g].load(a.ws + rev_member_ws(a) + a.w_off[g], wave, lane);
    for (int i = tid; i < NG * M * LDA; i += NT) lds[i] = 0.0f;

    const float sig_theta = snsde_sigmoid((a.params + (size_t)blockIdx.y * a.param_stride)[a.off_theta]);
    const bool mul_y = (a.no == 13 || a.no == 17 || a.no == 3 || a.no == 6 || a.no == 11);
    const bool yfun = (a.no >= 7 && a.no <= 10);
    const bool dsum = a.ds_part != nullptr && a.gt != nullptr;
    const bool tsum = dsum || yfun;       // d/d sigmoid(theta) wanted
    // field variants (tutorial-style fields, fields.py): f = tanh z | z | z y, g = the table row {y} itself, LipSwish / SiLU
    const bool variant = a.act_fn != 0 || a.f_out != 0 || a.g_out != 0;
    const bool g_raw = a.g_out == SNSDE_DIFFUSION_RAW;
    const float act_scale = a.act_fn == SNSDE_ACT_LIPSWISH ? 0.909f : 1.0f;
    const float sgt = g_raw ? 1.0f : sig_theta;       // d raw -> d g chain factor (RAW: none, and no theta gradient)
    const float rowf = row_ok ? 1.0f : 0.0f;
    const int rslot = a.row_out ? a.row_out[rowc] : -1;
    const float gfin = a.row_out ? a.grad_ys[goff] : 0.0f;
    float adj = 0.0f, th_acc = 0.0f;

    // g = tanh(sigmoid(theta) nan_to_num(raw)), raw = s(t) or s(t) y;  returns g, sets dg/dy, the clipped raw and its finiteness
    auto gfun = [&](float tv, float yy, float& gp, float& rc, bool& fin) {
        if (__builtin_expect(g_raw, 0)) {
            fin = true;
            rc = mul_y ? tv * yy : tv;
            gp = mul_y ? tv : 0.0f;
            return rc;
        }
        float q1 = mul_y ? tv : 0.0f, q2 = 0.0f;
        const float raw = yfun ? snsde_phi(a.no, yy, q1, q2) : (mul_y ? tv * yy : tv);
        fin = snsde_finite(raw);
        rc = snsde_nan_to_num(raw);
        const float g = fast_tanh(sig_theta * rc);
        gp = fin ? (1.0f - g * g) * sig_theta * q1 : 0.0f;
        return g;
    };
    auto quad_sum = [&](float v) {      // over the four rows of the tile (lanes differing in bits 0-1)
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));
        return v;
    };
    // one transposed chain: cotangent `cot` w.r.t. F of pass p (F = tanh(z * (GEO ? tanh(hin) : 1))); returns J_f^T cot for
    // the own element (the tanh(y) gate's direct term included)
    // relu masks of a pass are fetched while the previous chain runs (their HBM latency would otherwise sit between
    // the GEMMs of every chain)
    f32x4 mk[NG - 1], mk_next[NG - 1];
    auto load_masks = [&](int p, f32x4 (&dst)[NG - 1]) {
        if (writer) {
#pragma unroll
            for (int g = 0; g < NG - 1; ++g)
                dst[g] = *reinterpret_cast<const f32x4*>(a.act + uoff(p, SBH, (uint32_t)(NHID - g) + (a.act_fn != 0 ? (uint32_t)snsde_save::act_pre(NHID, 0, SNSDE_SRK, 0) : 0u), BH32) +
                                                         (uint32_t)(rowc * H + wave * 16 + fsub));     // (smooth activations: the PRE-activation slots)
        }
    };
    if (a.act_fn != 0) load_masks(3 * a.N - 1, mk);
    float acc_inv = 0.0f;          // accumulator column: 1 / g of the own column (additive table, constant over the step)
    // relu: the masks of pass p are the low NHID + 1 bits of its saved z (zbp; snsde_pack_signs) and every lane masks, hands on and
    // stores ITS OWN element of the all-reduced gradient; smooth activations: the writer lanes work on float4s of pre-activations
    const bool relu_bits = a.act_fn == 0;
    auto chain = [&](int p, float cot, float hin, float z, float F, uint32_t zbp) {
        if (!relu_bits && p > 0) load_masks(p - 1, mk_next);
        float ty = 1.0f;
        if constexpr (CF::GEO) ty = fast_tanh(hin);
        const float dzt = cot * (1.0f - F * F);
        float dz = dzt * ty;
        float direct = 0.0f;
        if constexpr (CF::GEO) direct = dzt * z * (1.0f - ty * ty);
        if (__builtin_expect(variant, 0)) {
            if (a.f_out == SNSDE_DRIFT_TIMES_Y) { dz = cot * hin; direct = cot * z; }
            else if (a.f_out == SNSDE_DRIFT_LINEAR) dz = cot;
        }
        if (__builtin_expect(a.acc_col >= 0, 0)) {
            // path-integral accumulator column: the owner's cotangent of ITS drift value of this pass (= of the KL rate u(t_s, H0_s))
            // is published to the tile row; the latent lanes add fbA d u / d F_j to their drift cotangent and fbA d u / d H0_j directly
            float* accb = lds + CF::ACC0;
            if (fcol == a.acc_col) accb[r] = cot;
            __syncthreads();
            const float fbA = accb[r];
            if (fcol < a.acc_col) {
                const float ue = (F - fmaf(a.acc_a, hin, a.acc_b)) * acc_inv * acc_inv * fbA;
                dz += ue;
                direct = fmaf(-a.acc_a, ue, direct);
            } else if (fcol == a.acc_col) {
                dz = 0.0f; direct = 0.0f;
            }
        }
        lds[r * LDA + fcol] = dz;
        if (a.delta && row_ok) (a.delta + uoff(p, NGBH))[goff] = dz;
        __syncthreads();
        float d = 0.0f;
        f32x4 acc[TPW], acc2[TPW];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            acc[0] = acc2[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            gemm<1, KUH, TPW>(wt[g], lds + g * M * LDA + r * LDA + 4 * s, acc, acc2);
            f32x4 v = acc[0] + acc2[0];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = row_ror_add(v[i]);
            if (g < NG - 1) {
                if (relu_bits) {
                    float mine = v[0];
                    mine = s1 ? v[1] : mine; mine = s2 ? v[2] : mine; mine = s3 ? v[3] : mine;
                    mine = ((zbp >> (NHID - g)) & 1u) ? mine : 0.0f;      // sign of act slot NHID - g of the own element
                    lds[(g + 1) * M * LDA + r * LDA + fcol] = mine;
                    if (a.delta && row_ok) (a.delta + uoff(p, NGBH, g + 1, BH32))[goff] = mine;
                } else if (writer) {
                    const f32x4 zsv = mk[g];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = v[i] * swish_grad(zsv[i], act_scale);
                    *reinterpret_cast<f32x4*>(lds + (g + 1) * M * LDA + r * LDA + wave * 16 + fsub) = v;
                    if (a.delta && row_ok)
                        *reinterpret_cast<f32x4*>(a.delta + uoff(p, NGBH, g + 1, BH32) + (uint32_t)(row * H + wave * 16 + fsub)) = v;
                }
                __syncthreads();
            } else {
                d = v[0];
                d = s1 ? v[1] : d; d = s2 ? v[2] : d; d = s3 ? v[3] : d;
            }
        }
#pragma unroll
        for (int g = 0; g < NG - 1; ++g) mk[g] = mk_next[g];
        return d + direct;
    };

    // per-step inputs (state, increments, saved pre-tanh drifts, table rows) are fetched one step ahead
    struct SrkIn { float y, ik, ik0, z0, z1, z2, t0v, t1v, t3v; };
    auto fetch = [&](int n, SrkIn& q) {
        const size_t so = uoff(n, BH32);
        q.y = (a.traj + so)[goff]; q.ik = (a.dW + so)[goff]; q.ik0 = (a.dU + so)[goff];
        q.z0 = (a.act + uoff(3 * n, SBH, CF::ZSLOT, BH32))[goff];
        q.z1 = (a.act + uoff(3 * n + 1, SBH, CF::ZSLOT, BH32))[goff];
        q.z2 = (a.act + uoff(3 * n + 2, SBH, CF::ZSLOT, BH32))[goff];
        q.t0v = q.t1v = q.t3v = 0.0f;
        if (a.gt) {
            const float* gp = a.gt + uoff(n, 4 * H, blockIdx.y, a.gt_stride) + fcol;      // (the member's table)
            q.t0v = gp[0]; q.t1v = gp[H]; q.t3v = gp[3 * H];
        }
    };
    SrkIn cur, nxt;
    fetch(a.N - 1, cur);

    for (int n = a.N - 1; n >= 0; --n) {
        nxt = cur;
        if (n > 0) fetch(n - 1, nxt);
        const float* st = a.step_tab + uoff(n, SNSDE_STEP_STRIDE);
        const float h = st[1], rdt = st[6];
        const int nout = __float_as_int(st[8]), kfirst = __float_as_int(st[9]);
        float carry = 0.0f;
        for (int k = kfirst; k < kfirst + nout; ++k) {
            const float w0 = a.out_w[2 * k], w1 = a.out_w[2 * k + 1];
            const float gk = a.row_out ? (rslot == k + 1 ? gfin : 0.0f) : (a.grad_ys + uoff(k + 1, BH32))[goff];
            if (w0 == 0.0f) adj += gk;
            else { adj = fmaf(w1, gk, adj); carry = fmaf(w0, gk, carry); }
        }
        if (row_ok && !a.adj0_only) (a.adj + uoff(n + 1, BH32))[goff] = adj;
        // ---- recompute the stage values of the step for the own element ----
        const float y = cur.y, ik = cur.ik, ik0 = cur.ik0;
        const uint32_t zclear = a.act_fn == 0 ? ~((1u << snsde_save::drift_sign_bits(NHID)) - 1u) : ~0u;      // (the sign bits are cleared before z is used)
        const uint32_t zb0 = __builtin_bit_cast(uint32_t, cur.z0), zb1 = __builtin_bit_cast(uint32_t, cur.z1), zb2 = __builtin_bit_cast(uint32_t, cur.z2);
        const float z0 = __builtin_bit_cast(float, zb0 & zclear), z1 = __builtin_bit_cast(float, zb1 & zclear), z2 = __builtin_bit_cast(float, zb2 & zclear);
        const float t0v = cur.t0v, t1v = cur.t1v, t3v = cur.t3v;
        if (__builtin_expect(a.acc_col >= 0, 0)) acc_inv = snsde_stable_inv(t0v);
        auto gate = [&](float hv) { return CF::GEO ? fast_tanh(hv) : 1.0f; };
        auto fout = [&](float z, float hv) {
            if (__builtin_expect(variant, 0)) {
                if (a.f_out == SNSDE_DRIFT_TIMES_Y) return z * hv;
                if (a.f_out == SNSDE_DRIFT_LINEAR) return z;
                return fast_tanh(z);
            }
            return fast_tanh(z * gate(hv));
        };
        float g0p, g1p, g2p, g3p, rc0, rc1, rc2, rc3;
        bool fi0, fi1, fi2, fi3;
        const float f0 = fout(z0, y);
        const float g0 = gfun(t0v, y, g0p, rc0, fi0);
        const float h01 = y + f0 * h;
        const float f1 = fout(z1, h01);
        const float h11 = y + 0.25f * f0 * h + SRK_B1_10 * g0 * rdt;
        const float g1 = gfun(t1v, h11, g1p, rc1, fi1);
        const float rh = 1.0f / h, rrdt = 1.0f / rdt;      // (as the forward: every `/ h`, `/ rdt` below multiplies)
        const float ik0h = ik0 * rh;
        const float h02 = y + 0.25f * f0 * h + 0.25f * f1 * h + (g0 + 0.5f * g1) * ik0h;
        const float f2 = fout(z2, h02);
        const float h12 = y + f0 * h + SRK_B1_20 * g0 * rdt;
        const float g2 = gfun(t3v, h12, g2p, rc2, fi2);
        const float h13 = y + 0.25f * f2 * h + (SRK_B1_30 * g0 + SRK_B1_31 * g1 + SRK_B1_32 * g2) * rdt;
        const float g3 = gfun(t1v, h13, g3p, rc3, fi3);
        // ---- reverse of the combination and of stage 3 / the diffusion half of stage 2 ----
        const float av = adj;
        const float ikk = 0.5f * (ik * ik - h);
        const float ikkk = (ik * ik * ik - 3.0f * h * ik) * (1.0f / 6.0f);
        const float a1 = ik, a2 = ikk * rrdt, a3 = ik0h, a4 = ikkk * rh;
        const float w0 = srk_w0(a1, a2, a3, a4);
        const float w1 = srk_w1(a1, a2, a3, a4);
        const float w2 = srk_w2(a1, a2, a3, a4);
        float yb = carry + av;
        float fb0 = av * (h * (1.0f / 6.0f)), fb1 = fb0, fb2 = av * (h * (2.0f / 3.0f));
        float gb0 = w0 * av, gb1 = w1 * av, gb2 = w2 * av;
        const float gb3 = a4 * av;
        float hb = gb3 * g3p;
        yb += hb; fb2 = fmaf(0.25f * h, hb, fb2);
        gb0 = fmaf(SRK_B1_30 * rdt, hb, gb0); gb1 = fmaf(SRK_B1_31 * rdt, hb, gb1); gb2 = fmaf(SRK_B1_32 * rdt, hb, gb2);
        hb = gb2 * g2p;
        yb += hb; fb0 = fmaf(h, hb, fb0); gb0 = fmaf(SRK_B1_20 * rdt, hb, gb0);
        // parameter side of G3 (slot 1, completed below with G1) and G2 (slot 3)
        float ds1 = 0.0f;
        if (tsum) {
            const float c3 = gb3 * (g_raw ? 1.0f : 1.0f - g3 * g3) * rowf, c2 = gb2 * (g_raw ? 1.0f : 1.0f - g2 * g2) * rowf;
            if (!g_raw) th_acc = fmaf(c3, rc3, fmaf(c2, rc2, th_acc));
            if (dsum) {
                ds1 = fi3 ? c3 * sgt * (mul_y ? h13 : 1.0f) : 0.0f;
                const float ds3 = quad_sum(fi2 ? c2 * sgt * (mul_y ? h12 : 1.0f) : 0.0f);
                if (r == 0) (a.ds_part + rev_member_ws(a))[((size_t)blockIdx.x * 4 * a.N + 4 * n + 3) * H + fcol] = ds3;
            }
        }
        // ---- stage 2: drift at (t0 + h/2, H0_2) ----
        float d = chain(3 * n + 2, fb2, h02, z2, f2, zb2);
        yb += d;
        fb0 = fmaf(0.25f * h, d, fb0); fb1 = fmaf(0.25f * h, d, fb1);
        gb0 = fmaf(ik0h, d, gb0); gb1 = fmaf(0.5f * ik0h, d, gb1);
        // ---- stage 1: diffusion at (t0 + h/4, H1_1), drift at (t0 + h, H0_1) ----
        hb = gb1 * g1p;
        yb += hb; fb0 = fmaf(0.25f * h, hb, fb0); gb0 = fmaf(SRK_B1_10 * rdt, hb, gb0);
        if (tsum) {
            const float c1 = gb1 * (g_raw ? 1.0f : 1.0f - g1 * g1) * rowf;
            if (!g_raw) th_acc = fmaf(c1, rc1, th_acc);
            if (dsum) {
                ds1 += fi1 ? c1 * sgt * (mul_y ? h11 : 1.0f) : 0.0f;
                ds1 = quad_sum(ds1);
                if (r == 0) (a.ds_part + rev_member_ws(a))[((size_t)blockIdx.x * 4 * a.N + 4 * n + 1) * H + fcol] = ds1;
            }
        }
        d = chain(3 * n + 1, fb1, h01, z1, f1, zb1);
        yb += d; fb0 = fmaf(h, d, fb0);
        // ---- stage 0: both at (t0, y) ----
        yb = fmaf(gb0, g0p, yb);
        if (tsum) {
            const float c0 = gb0 * (g_raw ? 1.0f : 1.0f - g0 * g0) * rowf;
            if (!g_raw) th_acc = fmaf(c0, rc0, th_acc);
            const float ds0 = dsum ? quad_sum(fi0 ? c0 * sgt * (mul_y ? y : 1.0f) : 0.0f) : 0.0f;
            if (dsum && r == 0) {
                (a.ds_part + rev_member_ws(a))[((size_t)blockIdx.x * 4 * a.N + 4 * n) * H + fcol] = ds0;
                (a.ds_part + rev_member_ws(a))[((size_t)blockIdx.x * 4 * a.N + 4 * n + 2) * H + fcol] = 0.0f;   // slot t0 + h/2: no diffusion evaluation
            }
        }
        d = chain(3 * n, fb0, y, z0, f0, zb0);
        adj = yb + d;
        cur = nxt;
    }
    if (row_ok) a.adj[goff] = adj + (a.row_out ? (rslot == 0 ? gfin : 0.0f) : a.grad_ys[goff]);
    if (tsum && a.dth_part) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) th_acc += __shfl_down(th_acc, off, 64);
        if (lane == 0) (a.dth_part + rev_member_ws(a))[blockIdx.x * CF::NW + wave] = th_acc;
    }
}

template <class CF>
int launch_rev_srk(const RevArgs& a, hipStream_t stream) {
    const size_t lds_bytes = (size_t)CF::RING0 * sizeof(float);      // (no weight ring in this kernel)
    const int members = a.members > 1 ? a.members : 1;      // (model ensembles: as launch_rev)
    const int grid = ((members > 1 ? a.member_rows : a.B) + CF::M - 1) / CF::M;
    hipLaunchKernelGGL(snsde_mfma_srk_reverse_kernel<CF>, dim3(grid, members), dim3(CF::NT), lds_bytes, stream, a);
    return hipGetLastError() == hipSuccess ? SNSDE_OK : SNSDE_ERR_LAUNCH;
}

// the forward kernel a plan runs (set by make_plan only; snsde_mfma_path reports it, snsde_mfma_launch dispatches on it)
enum class FwdKernel { w4, m4n, lean, lean_two_tile_h128, lean_two_tile_h256, lean_streamed_h256, general_m4, general_m16, lean_bf16 };

struct MfmaPlan {
    bool ok;
    bool shard_refused;    // !ok because the kernel planned for the whole problem (snsde_solve::global_rows) cannot run this shard:
                           // the route is then "no kernel" (SNSDE_ERR_UNSUPPORTED), never the generic family in its place
    bool samples_refused;  // !ok because the plan arrived at a kernel that does not map paths to input rows (snsde_solve::samples):
                           // "no kernel" as well
    bool members_refused;  // !ok because the plan arrived at a kernel that does not map rows to members (snsde_solve::members): the same
    FwdKernel kernel;
    int H, KUX, NHID, IO, FL, TPW, NW, FOLD, NN, SRK;
    int LEAN, KUXT;    // lean M4 kernel (snsde_m4_kernel.h) and its 16-wide k-blocks of [X(t) | sin t, cos t]
    int LEAN_SPEC;     // kernel == lean: 0 general instantiation, 1 / 2 the compile-time mode CfgSpec<.., GEO = 0 / 1>
    int M4N, KUXN;     // diffusion nets under SRK / Milstein (snsde_m4n_kernel.h) and its control k-blocks (0: latent-only drift)
    int srk_tab_off;   // expanded (3N-row) step table of the SRK variant inside the workspace
    int n_bias_rows;
    int fold_b_in, fold_b_init, fold_b_emb, fold_emb_w, fold_bias_tmp;
    int n_layers;
    MfmaLayerPack layer[MAXL];
    int bias_off, gt_off, total_floats;
};

// the adjoint kernel a plan runs (set by make_rev_plan only; snsde_mfma_backward_launch dispatches on it)
enum class RevKernel {
    w4_fused,        // wave-pair adjoint with the weight gradients inside (snsde_w4_rev_launch): no delta planes
    m4n_srk,         // SRK through a diffusion net (snsde_m4n_rev_kernel.h)
    m4n_milstein,    // Milstein through a diffusion net (snsde_m4n_mil_rev_kernel.h)
    general_srk,     // SRK adjoint of the general kernel (launch_rev_srk, 4-row tiles)
    two_tile_h256,   // H = 256, two tiles per wave, a quarter of the transposed weights resident (snsde_m4s2_rev_kernel.h)
    general          // Euler / Milstein adjoint of the general kernel on 4- or 16-row tiles (dispatch_rev)
};

struct RevPlan {
    bool ok;
    RevKernel kernel;
    int H, NHID, GEO, FL, NW, NN, SRK, IO0, n_layers, fold_tmp, total_floats, emb;
    int M4N;                    // weight layout of the diffusion-net adjoints: 1 m4n_srk, 2 m4n_milstein (+ the forward-layout net), 0 else
    int nwg;                    // workgroups of the adjoint launch
    size_t ds_off, dth_off;     // diffusion-side partial sums inside the backward workspace (0 = none)
    size_t w4_gpart_off;        // kernel == w4_fused: the per-tile weight-gradient blocks, behind the plan's own floats
    size_t workspace_floats;    // the whole backward workspace (total_floats, + the blocks at w4_gpart_off)
    MfmaLayerPack layer[MAXL];
};

// The adjoint of a solve, decided once per entry point (route_backward, snsde_api.hip): the mode snsde_backward_supported reports
// (0 none, 1 MFMA adjoint, 2 generic adjoint), the forward's plan - the one its launch ran with - and the adjoint's plan.
// Mode 1 runs rp; the plans are filled in whatever the mode (snsde_backward_workspace_bytes sizes for rp wherever it is ok).
// members > 1 (a model ensemble under SNSDE_FLAG_ENSEMBLE_GRAD): fp is the ensemble forward's plan, rp the adjoint's plan of ONE member
// run alone as a shard of the whole (batch / M rows: its nwg, its offsets) - every member's block of the backward workspace is laid
// out by it, bws_stride floats apart (snsde_member_bws_stride); fws_stride: floats between the members' blocks of the forward
// workspace (snsde_member_ws_stride).  One model: members = 1, strides 0.
struct BackwardRoute { int mode; MfmaPlan fp; RevPlan rp; int members; size_t bws_stride, fws_stride; };

// Which 4-row-tile configurations the lean kernel (snsde_m4_kernel.h) takes: its resident weights plus one layer's B
// operands must fit the 256-register budget of two waves per SIMD WITHOUT spilling (its asm-issued loads land in
// registers the compiler believes are already written, so a spill of one of them would save stale data).  Measured on the
// instantiations: no spill while  weight registers + the loop-carried [X | tau] operands  <= 112 (K2: 104 + 8, 253 VGPRs);
// build.py fails the build if an instantiation spills.  KUXT = 16-wide k-blocks of [X(t) | sin t, cos t].
__host__ __device__ constexpr bool lean_fits(int H, int NHID, int KUXT, bool YIN) {
    // streamed-weight variant (snsde_m4s_kernel.h); (NHID 0, KUXT 3) would spill two registers in training mode
    if (H == 256) return YIN && NHID <= 2 && KUXT <= 3 && !(NHID == 0 && KUXT == 3);
    return (H == 32 || H == 64 || H == 128) && 4 * (KUXT + (YIN ? H / 16 : 0) + (NHID + 1) * (H / 16)) + 4 * KUXT <= (YIN ? 112 : 104);
}
// training-mode instantiations of the smooth-activation variants (they also store the pre-activations)
__host__ __device__ constexpr bool lean_act_save_fits(int H, int NHID, int KUXT) {
    return H <= 128 && lean_fits(H, NHID, KUXT, true) && 4 * (KUXT + H / 16 + (NHID + 1) * (H / 16)) + 4 * KUXT <= 104;
}
// largest KUXT a (input_option, KUX) class of the general kernel can meet (KUX = 5: 33..80 control channels)
__host__ __device__ constexpr int lean_kuxt_max(int IO, int KUX) {
    const bool usex = (IO == 0 || IO == 2 || IO == 4 || IO == 6), timef = IO >= 3;
    return KUX == 5 ? 6 : (usex ? (timef ? 3 : 2) : (timef ? 1 : 0));
}

template <int H, int KUX, int NHID, int IO, int FL, int NN>
int dispatch_var(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) {
    constexpr bool emb = (IO == 2 || IO == 4 || IO == 6);
    // 4-row tiles with an elementwise diffusion at H = 32 / 64 / 128 run on the lean kernel (snsde_m4_kernel.h;
    // snsde_mfma_launch dispatches them before coming here): not instantiated twice
    constexpr bool lean_cov = (FL == 1 && NN == 0 && lean_fits(H, NHID, lean_kuxt_max(IO, KUX), IO != 0));
    if constexpr (emb) {
        if (p.FOLD) {
            if constexpr (lean_cov) return SNSDE_ERR_UNSUPPORTED;
            else return launch_cfg<Cfg<H, KUX, NHID, IO, FL, 1, 1, NN>>(a, st);
        }
        if constexpr (NN > 0) return SNSDE_ERR_UNSUPPORTED;   // diffusion nets behind a control embedding: folded layer only
        if constexpr (NHID > 1) return SNSDE_ERR_UNSUPPORTED;   // exact-order variant: diagnostic, NL <= 2 only
    }
    if constexpr (!emb && lean_cov) return SNSDE_ERR_UNSUPPORTED;
    else if constexpr (!emb || (NHID <= 1 && NN == 0))
        return launch_cfg<Cfg<H, KUX, NHID, IO, FL, 1, 0, NN>>(a, st);
    return SNSDE_ERR_UNSUPPORTED;
}

// Instantiated configurations: input_option 1..6, up to 3 hidden `linears` (NL <= 4), C <= 32 (two 16-wide k-blocks) or
// C <= 80 (five, folded first layer),
// diffusion nets (noise_option 14/15/18/19) for the latent-only drifts (input_option 1, 3, 5).
template <int H, int FL>
int dispatch_io(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) {
#ifdef SNSDE_DEV_SUBSET   // development builds: the headline configuration only
    if (p.IO == 4 && p.NHID == 1 && p.NN == 0) return dispatch_var<H, 2, 1, 4, FL, 0>(p, a, st);
    return SNSDE_ERR_UNSUPPORTED;
#else
    if (p.SRK) {           // SRID2 stepper: folded first layer, elementwise diffusions; 4-row tiles, and 16-row tiles at H = 64 / 128 (C <= 32)
        if constexpr (FL == 1 || H == 64 || H == 128) {
#define SNSDE_SRKC(IO_, NHID_) \
    if (p.IO == IO_ && p.NHID == NHID_ && p.KUX != 5) return launch_cfg<Cfg<H, (IO_ % 2 == 0 ? 2 : 1), NHID_, IO_, FL, 1, (IO_ != 0 ? 1 : 0), 0, 1>>(a, st); \
    if (FL == 1 && p.IO == IO_ && p.NHID == NHID_ && p.KUX == 5 && IO_ % 2 == 0 && IO_ != 0 && NHID_ <= 2) return launch_cfg<Cfg<H, (IO_ % 2 == 0 && IO_ != 0 && NHID_ <= 2 ? 5 : 1), NHID_, IO_, 1, 1, 1, 0, 1>>(a, st);
#define SNSDE_SRKS(IO_) SNSDE_SRKC(IO_, 0) SNSDE_SRKC(IO_, 1) SNSDE_SRKC(IO_, 2) SNSDE_SRKC(IO_, 3)
            SNSDE_SRKS(0) SNSDE_SRKS(1) SNSDE_SRKS(2) SNSDE_SRKS(3) SNSDE_SRKS(4) SNSDE_SRKS(5) SNSDE_SRKS(6)
#undef SNSDE_SRKS
#undef SNSDE_SRKC
        }
        return SNSDE_ERR_UNSUPPORTED;
    }
#define SNSDE_WIDE(IO_, NHID_) \
    if (p.IO == IO_ && p.NHID == NHID_) { \
        if constexpr (FL == 1 && lean_fits(H, NHID_, 6, IO_ != 0)) return SNSDE_ERR_UNSUPPORTED;   /* lean kernel */ \
        else return launch_cfg<Cfg<H, 5, NHID_, IO_, FL, 1, 1, 0>>(a, st); }
    if (p.KUX == 5) {      // wide control paths (32 < C <= 80, e.g. the sepsis channels): folded first layer only
        {
        SNSDE_WIDE(0, 0) SNSDE_WIDE(0, 1) SNSDE_WIDE(0, 2) SNSDE_WIDE(0, 3)
        SNSDE_WIDE(2, 0) SNSDE_WIDE(2, 1) SNSDE_WIDE(2, 2) SNSDE_WIDE(2, 3)
        SNSDE_WIDE(4, 0) SNSDE_WIDE(4, 1) SNSDE_WIDE(4, 2) SNSDE_WIDE(4, 3)
        SNSDE_WIDE(6, 0) SNSDE_WIDE(6, 1) SNSDE_WIDE(6, 2) SNSDE_WIDE(6, 3)
        return SNSDE_ERR_UNSUPPORTED;
        }
    }
#undef SNSDE_WIDE
#define SNSDE_CASE(IO_, NHID_, NN_) \
    if (p.IO == IO_ && p.NHID == NHID_ && p.NN == NN_) return dispatch_var<H, (IO_ % 2 == 0 ? 2 : 1), NHID_, IO_, FL, NN_>(p, a, st);
#define SNSDE_CASES(IO_, NN_) SNSDE_CASE(IO_, 0, NN_) SNSDE_CASE(IO_, 1, NN_) SNSDE_CASE(IO_, 2, NN_) SNSDE_CASE(IO_, 3, NN_)
    SNSDE_CASES(0, 0) SNSDE_CASES(0, 1) SNSDE_CASES(0, 2)
    SNSDE_CASES(2, 0) SNSDE_CASES(4, 0) SNSDE_CASES(6, 0)
    SNSDE_CASES(1, 0) SNSDE_CASES(3, 0) SNSDE_CASES(5, 0)
    SNSDE_CASES(1, 1) SNSDE_CASES(3, 1) SNSDE_CASES(5, 1) SNSDE_CASES(1, 2) SNSDE_CASES(3, 2) SNSDE_CASES(5, 2)
    SNSDE_CASES(2, 1) SNSDE_CASES(4, 1) SNSDE_CASES(6, 1) SNSDE_CASES(2, 2) SNSDE_CASES(4, 2) SNSDE_CASES(6, 2)
#undef SNSDE_CASES
#undef SNSDE_CASE
    return SNSDE_ERR_UNSUPPORTED;
#endif
}

template <int H, int FL>
int dispatch_rev(const RevPlan& p, const RevArgs& a, hipStream_t st) {
#ifdef SNSDE_DEV_SUBSET
    if (p.NHID == 1 && !p.GEO) return launch_rev<CfgR<H, 1, 0, FL>>(a, st);
    return SNSDE_ERR_UNSUPPORTED;
#else
    if (p.SRK) {
        if constexpr (FL == 1) {
#define SNSDE_RSRK(NH_) if (p.NHID == NH_) return p.GEO ? launch_rev_srk<CfgR<H, NH_, 1, 1>>(a, st) : launch_rev_srk<CfgR<H, NH_, 0, 1>>(a, st);
            SNSDE_RSRK(0) SNSDE_RSRK(1) SNSDE_RSRK(2) SNSDE_RSRK(3)
#undef SNSDE_RSRK
        }
        return SNSDE_ERR_UNSUPPORTED;
    }
    if (p.IO0) {
#define SNSDE_R0(NH_) if (p.NHID == NH_) { \
        if (p.NN == 1) return launch_rev<CfgR<H, NH_, 0, FL, 1, 1>>(a, st); \
        if (p.NN == 2) return launch_rev<CfgR<H, NH_, 0, FL, 2, 1>>(a, st); \
        return launch_rev<CfgR<H, NH_, 0, FL, 0, 1>>(a, st); }
        SNSDE_R0(0) SNSDE_R0(1) SNSDE_R0(2) SNSDE_R0(3)
#undef SNSDE_R0
        return SNSDE_ERR_UNSUPPORTED;
    }
#define SNSDE_RCASE(NH_) if (p.NHID == NH_) { \
        if (p.NN == 1) return p.GEO ? launch_rev<CfgR<H, NH_, 1, FL, 1>>(a, st) : launch_rev<CfgR<H, NH_, 0, FL, 1>>(a, st); \
        if (p.NN == 2) return p.GEO ? launch_rev<CfgR<H, NH_, 1, FL, 2>>(a, st) : launch_rev<CfgR<H, NH_, 0, FL, 2>>(a, st); \
        return p.GEO ? launch_rev<CfgR<H, NH_, 1, FL>>(a, st) : launch_rev<CfgR<H, NH_, 0, FL>>(a, st); }
    SNSDE_RCASE(0) SNSDE_RCASE(1) SNSDE_RCASE(2) SNSDE_RCASE(3)
#undef SNSDE_RCASE
    return SNSDE_ERR_UNSUPPORTED;
#endif
}

// per-hidden-size, per-flavour entry points (snsde_mfma_h*.hip: one translation unit each, compiled in parallel)
int dispatch_fwd_m16_h16(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_fwd_m4_h16(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_rev_h16(const RevPlan& p, const RevArgs& a, hipStream_t st);
int dispatch_rev_h256_two_tile(const RevPlan& p, const RevArgs& a, hipStream_t st);   // snsde_m4s2_rev_kernel.h
bool m4s2_rev_instantiated(int nhid, bool geo);                                         // (its instantiation list)
int dispatch_fwd_m16_h32(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_fwd_m4_h32(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_rev_h32(const RevPlan& p, const RevArgs& a, hipStream_t st);
int dispatch_fwd_m16_h64(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_fwd_m4_h64(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_rev_h64(const RevPlan& p, const RevArgs& a, hipStream_t st);
int dispatch_fwd_m16_h128(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_fwd_m4_h128(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_rev_h128(const RevPlan& p, const RevArgs& a, hipStream_t st);
int dispatch_fwd_m16_h256(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_fwd_m4_h256(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_rev_h256(const RevPlan& p, const RevArgs& a, hipStream_t st);

}  // namespace snsde_mfma
