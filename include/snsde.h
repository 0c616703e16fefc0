/*
 * snsde.h - C ABI of the MI355X-native Neural-SDE integration engine (libsnsde.so).
 *
 * The reference (yongkyung-oh/Stable-Neural-SDEs) is pure Python: it has no native interface.
 * The entry points below are what a binding for the hot path
 *
 *     torchsde.sdeint(sde=Diffusion_model, y0, ts, dt, method=...)
 *         benchmark_classification/models_sde/neuralsde.py:71-82   (call site, "A1" in SURVEY.md 8a)
 *         benchmark_forecasting/models_sde/neuralsde.py:71-82,145-156
 *         torch-ists/torch_ists/diff_module/NSDE/nsde_model.py:63-74
 *     torchcde.CubicSpline(coeffs, times).evaluate(t)
 *         benchmark_classification/models_sde/neuralsde.py:181-184, 296   (set_X / f)
 *         benchmark_classification/controldiffeq/interpolate.py:263-276    (vendored twin)
 *
 * would bind.  Plain C types, device pointers and sizes only; no torch types.  Every buffer is
 * caller-owned.  Launch functions only ENQUEUE work on the given HIP stream: they never allocate,
 * never synchronise and never throw, so a solve can be captured into a hipGraph.  All functions
 * return SNSDE_OK (0) or a negative error code (snsde_strerror()).  The library is stateless and
 * re-entrant; concurrent calls on different streams / devices are legal.
 *
 * All tensors are float32, row-major, contiguous.
 */
#ifndef SNSDE_H
#define SNSDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  2 (round 4): every descriptor struct starts with `struct_size` = sizeof(the struct) as the CALLER compiled it;
 * the library compares it with its own sizeof and refuses a mismatch with SNSDE_ERR_ABI, so a binding built against an older
 * header (the structs grew fields in rounds 2 - 3 while the version stayed 1) fails loudly instead of being read past its end.
 * snsde_abi_check() lets a binding verify all of its struct sizes once, at load time.                                        */
#define SNSDE_VERSION 2

/* exported entry points: the library is built with -fvisibility=hidden, only these names are in its dynamic symbol table */
#define SNSDE_API __attribute__((visibility("default")))

enum {
    SNSDE_OK = 0,
    SNSDE_ERR_NULL = -1,         /* required pointer is NULL                                  */
    SNSDE_ERR_DIMS = -2,         /* non-positive / inconsistent dimension                      */
    SNSDE_ERR_OPTION = -3,       /* input_option not in 0..6 or noise_option not in 0..19      */
    SNSDE_ERR_UNSUPPORTED = -4,  /* valid request this build has no kernel for                 */
    SNSDE_ERR_WORKSPACE = -5,    /* workspace too small (see snsde_workspace_bytes)             */
    SNSDE_ERR_LDS = -6,          /* configuration exceeds the 160 KiB LDS budget of a CU        */
    SNSDE_ERR_TS = -7,           /* ts not strictly increasing / dt <= 0 / no fp32 progress     */
    SNSDE_ERR_LAUNCH = -8,       /* hipLaunchKernel reported an error                           */
    SNSDE_ERR_INDEX = -9,        /* index out of range                                          */
    SNSDE_ERR_ABI = -10          /* struct_size / version of the caller's binding differs from the library's */
};

enum { SNSDE_EULER = 0, SNSDE_MILSTEIN = 1, SNSDE_SRK = 2 /* SRID2, strong order 1.5, diagonal noise */ };

/* kernel selection (for tests / benchmarking); 0 lets the library choose */
enum {
    SNSDE_KERNEL_AUTO = 0,      /* MFMA fast path when the configuration is covered, else generic  */
    SNSDE_KERNEL_GENERIC = 1,   /* VALU kernel: every (input_option, noise_option), any dims        */
    SNSDE_KERNEL_MFMA = 2,      /* MFMA fast path, tile flavour chosen from the batch size          */
    SNSDE_KERNEL_MFMA_M16 = 3,  /* 16-row tiles (v_mfma_f32_16x16x4_f32)                            */
    SNSDE_KERNEL_MFMA_M4 = 4,   /* 4-row tiles  (v_mfma_f32_4x4x1_16b_f32)                          */
    SNSDE_KERNEL_MFMA_W4 = 5    /* 4-row tiles owned by ONE wave (H = 64 with a diffusion net, Euler): drift wave + net wave */
};

/* flags: REUSE_PREPARED skips the weight packing / time-table kernels; legal when `params`,
 * `step_tab` and `workspace` are unchanged since the previous call that ran them (e.g. every
 * batch of an evaluation epoch, or graph replays between optimizer steps). */
enum {
    SNSDE_FLAG_REUSE_PREPARED = 1,
    /* keep the reference's operation order yy = linear_in(..); z = emb(cat[yy, Xt]) on the MFMA path.  Default
     * (flag clear): emb o linear_in and emb o initial_network are pre-multiplied once per solve (there is no
     * non-linearity between them, neuralsde.py:200-210), which removes one layer and one barrier per step;
     * the result differs from the unfused order by float32 round-off only. */
    SNSDE_FLAG_EXACT_ORDER = 2,
    /* H = 256 on 4-row tiles: keep the fully streamed kernel (sixteen waves, every weight through the LDS ring each step) instead of
     * the two-tiles-per-wave kernel that holds a quarter of every layer in registers.  Same results bit for bit (same MFMA chains);
     * exists for A/B measurements and the bit-identity test. */
    SNSDE_FLAG_STREAM_ALL = 4,
    /* H = 128 on 4-row tiles (Euler / Milstein, elementwise diffusions, relu fields): four waves of two tiles, one wave per SIMD with
     * the whole register file (snsde_m4t_kernel.h), instead of the eight-wave lean kernel.  Same results bit for bit.  An A/B switch:
     * measured slower at the K2 shape, so it is opt-in. */
    SNSDE_FLAG_TWO_TILE = 8,
    /* Inference only, opt-in: bf16 MFMA operands on the lean 4-row-tile kernel (SNSDE_PATH_LEAN_BF16; the reference's
     * Diffusion_model fields with elementwise diffusions, Euler / Milstein, H = 64 / 128).  Only the two operands of every
     * matrix instruction are rounded to bf16 (nearest even): the layer weights and the layer inputs [X(t) | sin t, cos t], y and
     * the hidden activations.  The state, accumulators, biases, tanh, the diffusion, Milstein's term, the increments, X(t), the
     * update and the output interpolation stay f32.  SNSDE_ERR_UNSUPPORTED (never an f32 kernel instead) for any other
     * configuration, with training outputs (act_save, stage_save, traj, dW_out, dU_out), and from every backward entry point
     * (snsde_backward_supported returns 0) - unless SNSDE_FLAG_BF16_GRAD opts in to training. */
    SNSDE_FLAG_BF16_OPERANDS = 16,
    /* Run the lean 4-row-tile kernel's general instantiation even where a compile-time specialised one covers the launch
     * (snsde_lean_variant).  Same results bit for bit; exists for A/B measurements and the bit-identity test. */
    SNSDE_FLAG_LEAN_GENERAL = 32,
    /* Opt-in: a solve of `samples` = S > 1 paths per input row may be differentiated (snsde_solve.samples, last paragraph).  No
     * effect when samples <= 1.  Together with SNSDE_FLAG_BF16_OPERANDS (an inference-only forward): SNSDE_ERR_UNSUPPORTED. */
    SNSDE_FLAG_SAMPLE_GRAD = 64,
    /* Opt-in: training through the bf16-operand forward.  Meaningful only together with SNSDE_FLAG_BF16_OPERANDS (alone: no
     * effect).  The forward then accepts act_save, traj and dW_out on SNSDE_PATH_LEAN_BF16 (training-mode instantiations of the same
     * kernel: the states are the inference kernel's bit for bit, the planes hold the f32 values in front of the operand rounding),
     * and the backward entry points return the gradient of the function that forward computed, with the rounding q treated as the
     * identity in the backward pass (straight-through), in f32 arithmetic: for a layer z = q(W) q(x) + b
     *     dL/dx = q(W)^T delta,   dL/dW = delta (x) q(x),   dL/db = sum delta
     * - the adjoint multiplies the rounded weights (the folded products emb . linear_in of input_option 2 / 4 / 6 rounded after
     * folding, as in the forward), the weight-gradient pass rounds its X operands (act_save slots, traj, the control-path columns and
     * sin t, cos t after evaluation) while staging them; the gradient of a folded product reaches emb, linear_in and
     * initial_network through the f32 fold.  Masks, tanh', the diffusion, Milstein's term and the Philox regeneration have no matrix
     * operand and are the f32 path's.  snsde_backward_supported == 1 where the forward plan is the bf16 lean kernel (Euler /
     * Milstein, elementwise diffusions, H = 64 / 128, the reference's fields, kl_column1 == 0) and no noise_table is supplied;
     * 0 (never an f32 kernel, never mode 2) for everything else, samples > 1 included.  stage_save / dU_out stay refused, and
     * snsde_coeff_gradients returns SNSDE_ERR_UNSUPPORTED under bf16 operands with or without this flag. */
    SNSDE_FLAG_BF16_GRAD = 128,
    /* Opt-in: a model ensemble (snsde_solve.members = M > 1) may be differentiated (snsde_solve.members, last paragraph).  No
     * effect when members <= 1.  Together with SNSDE_FLAG_BF16_OPERANDS (an inference-only forward): SNSDE_ERR_UNSUPPORTED. */
    SNSDE_FLAG_ENSEMBLE_GRAD = 256,
    /* Opt-in: sample paths of a model ensemble - members = M > 1 together with samples = S > 1 in one solve (M x S paths per
     * input row; snsde_solve.members, the paragraph on sample paths).  No effect when members <= 1 or samples <= 1; without it
     * the combination stays SNSDE_PATH_NONE / SNSDE_ERR_UNSUPPORTED.  Training through it needs this flag together with
     * SNSDE_FLAG_ENSEMBLE_GRAD and SNSDE_FLAG_SAMPLE_GRAD: each of the three keeps its own meaning. */
    SNSDE_FLAG_ENSEMBLE_SAMPLES = 512,
    /* Opt-in: a model ensemble (snsde_solve.members = M > 1) on the kernels of the diffusion nets (noise_option 14 / 15 / 18 / 19)
     * - the wave pairs (SNSDE_FWD_W4) and the diffusion-net 4-row tiles (SNSDE_FWD_M4N); snsde_solve.members, last paragraph.  No
     * effect when members <= 1; without it a plan that arrives at these kernels stays SNSDE_PATH_NONE for M > 1.  Inference only:
     * with training planes, with or without SNSDE_FLAG_ENSEMBLE_GRAD, such an ensemble stays SNSDE_PATH_NONE and
     * snsde_backward_supported stays 0 (SNSDE_FLAG_ENSEMBLE_NETS_GRAD opts in for the wave pairs).  Sample paths of such an
     * ensemble need SNSDE_FLAG_ENSEMBLE_SAMPLES as well. */
    SNSDE_FLAG_ENSEMBLE_NETS = 1024,
    /* Opt-in: training through a model ensemble on the wave pairs (SNSDE_FWD_W4 / SNSDE_REV_W4_FUSED: H = 64, diffusion nets, Euler
     * or SRK; snsde_solve.members, last paragraph).  Meaningful only with members > 1 and both SNSDE_FLAG_ENSEMBLE_NETS and
     * SNSDE_FLAG_ENSEMBLE_GRAD set; each of the three keeps its own meaning.  Alone, or with only one of the other two, it changes
     * no answer. */
    SNSDE_FLAG_ENSEMBLE_NETS_GRAD = 2048,
    /* Opt-in: a continued solve (snsde_solve_forward_at with step_offset != 0) may be differentiated.  With it the forward accepts
     * the training planes at every offset, and the backward entry points' _at forms take the same offset (snsde_solve_forward_at,
     * last paragraph).  No plan reads it and at step_offset == 0 it changes nothing. */
    SNSDE_FLAG_RESUME_GRAD = 4096
};

/* Variants of the vector field beyond the benchmark Diffusion_model: the tutorial's Neural LSDE / LNSDE / GSDE fields
 * (tutorial notebooks, cell 7: MLPs with LipSwish activations, raw time feature, un-squashed drift and diffusion) map
 * onto the same fused step with these four switches (all 0 = the reference Diffusion_model, neuralsde.py:186-307).   */
enum { SNSDE_ACT_RELU = 0, SNSDE_ACT_LIPSWISH = 1 /* 0.909 silu(x) */, SNSDE_ACT_SILU = 2 };
enum { SNSDE_DRIFT_TANH = 0 /* f = tanh(z) (z * tanh(y) first for input_option 5/6) */, SNSDE_DRIFT_LINEAR = 1 /* f = z */,
       SNSDE_DRIFT_TIMES_Y = 2 /* f = z * y */ };
enum { SNSDE_DIFFUSION_TANH = 0 /* g = tanh(sigmoid(theta) nan_to_num(raw)) */, SNSDE_DIFFUSION_RAW = 1 /* g = raw */,
       SNSDE_DIFFUSION_RAW_NET = 2 /* noise_option 18 / 19 only: g = raw AND the net's last layer is not rectified (the tutorial's */
                                   /* NeuralSDEFunc: g = g_net(noise_in([t, y])), an MLP that ends in a Linear)                  */ };
enum { SNSDE_TIME_SINCOS = 0 /* linear_in sees [sin t, cos t, y] */, SNSDE_TIME_RAW = 1 /* [t, 0, y] */ };

/* Shape of a Diffusion_model: neuralsde.py:123-179 constructor arguments (+ the variant switches above). */
typedef struct snsde_model {
    int32_t input_channels;          /* C  */
    int32_t hidden_channels;         /* H  */
    int32_t hidden_hidden_channels;  /* HH (the reference requires HH == H whenever emb is used) */
    int32_t num_hidden_layers;       /* NL >= 1; there are NL-1 `linears` */
    int32_t input_option;            /* 0..6  */
    int32_t noise_option;            /* 0..19 */
    int32_t activation;              /* SNSDE_ACT_*        (0 for the reference's models) */
    int32_t drift_output;            /* SNSDE_DRIFT_*      (0 ...)                        */
    int32_t diffusion_output;        /* SNSDE_DIFFUSION_*  (0 ...)                        */
    int32_t time_feature;            /* SNSDE_TIME_*       (0 ...)                        */
} snsde_model;

/* ---- parameter block ------------------------------------------------------------------------
 * The engine reads ONE flat float32 buffer holding every parameter of the Diffusion_model in
 * state_dict order with the reference's names and nn.Linear layout (weight (out,in) row-major):
 *   theta (1,1) | sigma (1) | sigma_diag (H) | initial_network.{weight (H,C),bias} |
 *   linear_in.{weight (HH, H or H+2),bias} | emb.{weight (H,2H),bias} | linears.i.{weight,bias} |
 *   linear_out.{weight (H,HH),bias} | noise_t[.0/.2].* | noise_y[.0/.2].*
 * (neuralsde.py:142-179).  These functions describe that layout so a host can fill it. */
SNSDE_API int     snsde_param_count(const snsde_model* m);                 /* number of tensors, or <0 */
SNSDE_API int64_t snsde_param_numel(const snsde_model* m);                 /* total floats, or <0      */
SNSDE_API int     snsde_param_info(const snsde_model* m, int index, char* name, int name_cap,
                         int64_t* offset, int32_t* rows, int32_t* cols);

/* ---- fixed-step time grid (host, CPU) --------------------------------------------------------
 * torchsde 0.2.5 BaseSDESolver.integrate bookkeeping, emulated in float32:
 *   curr = ts[0]; for out_t in ts[1:]: while curr < out_t: next = min(curr + dt, ts[-1]); step
 * plus, per step, the spline interval of t0 on the knot grid `times`
 * (interpolate.py:263-268: idx = clamp(#{j: times[j] < t} - 1, 0, L-2), frac = t - times[idx]).
 *
 * step_tab row (SNSDE_STEP_STRIDE floats): [0] t0, [1] h = t1-t0, [2] sin(t0), [3] cos(t0), [4] frac,
 * [5] idx (int32 bit pattern), [6] sqrt(h), [7] t1, [8] number of outputs emitted after this step
 * (int32 bits), [9] index k of the first of them (int32 bits), [10..11] zero.
 * out_step[k] = index of the solver step after which output k+1 is emitted; out_w[2k], out_w[2k+1] =
 * linear_interp weights (t1-t)/(t1-t0), (t-t0)/(t1-t0).                                          */
#define SNSDE_STEP_STRIDE 12
SNSDE_API int snsde_grid_count(const float* ts, int32_t n_out, double dt, int32_t* n_steps);
SNSDE_API int snsde_grid_build(const float* ts, int32_t n_out, double dt, const float* times, int32_t knots,
                     int32_t n_steps, float* step_tab, int32_t* out_step, float* out_w);
/* Stage times of the SRK scheme: per solver step the four evaluation times t0 + c*h, c = 0, 1/4, 1/2, 1
 * (float32 arithmetic as torchsde's `t0 + c * dt`), each as SNSDE_SRK_STRIDE floats:
 * t, sin t, cos t, frac, idx (int32 bits), 0, 0, 0.   srk_tab is (n_steps, 4, SNSDE_SRK_STRIDE). */
#define SNSDE_SRK_STRIDE 8
SNSDE_API int snsde_grid_srk_build(const float* step_tab, int32_t n_steps, const float* times, int32_t knots, float* srk_tab);

/* ---- the solve --------------------------------------------------------------------------------
 * Replaces torchsde.sdeint(sde=Diffusion_model, y0, ts, dt, method) (neuralsde.py:78-82):
 * every solver step fuses X(t) (A10), f (A7), g (A8), the Brownian increment (A5) and the
 * Euler / Milstein update (A4/A6) for a tile of batch rows; rows are independent.            */
typedef struct snsde_solve {
    uint32_t struct_size;  /* = sizeof(snsde_solve) of the caller's header (SNSDE_ERR_ABI otherwise)              */
    snsde_model model;
    int32_t  batch;        /* B: rows on this device                                             */
    int32_t  knots;        /* L: len(times); coeffs has L-1 intervals                            */
    int32_t  n_steps;      /* N (snsde_grid_count)                                               */
    int32_t  n_out;        /* T = len(ts)                                                        */
    int32_t  method;       /* SNSDE_EULER | SNSDE_MILSTEIN | SNSDE_SRK                           */
    int32_t  kernel;       /* SNSDE_KERNEL_*                                                     */
    int32_t  flags;        /* SNSDE_FLAG_*                                                       */
    int32_t  members;      /* M: models of one architecture solved by this call (0 or 1: one model, today's behaviour).   */
                           /* M > 1, a model ensemble (inference only): `batch` counts ALL rows, member-major - row         */
                           /* r = m Bm + b with Bm = batch / M rows per member; `params` is (M, snsde_param_numel)          */
                           /* contiguous, member m reads block m; `coeffs` stays (Bm, L-1, 4C) and is shared - row r reads  */
                           /* coefficient row r - m Bm; y0, ys, dW, dU and row_out stay per row, the Philox counter stays   */
                           /* (row_offset + r, ..).  Member m's rows equal, bit for bit, the ordinary solve of member m     */
                           /* alone run as a shard of the whole: members = 0, batch = Bm, params = block m, row_offset +    */
                           /* m Bm, global_rows = this call's global_rows (or, where that is 0, this call's batch).         */
                           /* SNSDE_ERR_DIMS: members < 0, batch % M != 0, Bm % 4 != 0 (a 4-row tile never straddles two    */
                           /* members, and no member has a ragged tail).  SNSDE_ERR_UNSUPPORTED (snsde_backward_supported   */
                           /* == 0): samples > 1, z0_weight, noise_table, kl_column1 != 0, act_save / stage_save / traj /   */
                           /* dW_out / dU_out, every backward entry point, snsde_eval_fg.  Kernels: the lean 4-row-tile     */
                           /* kernel (general, specialised, bf16; Euler / Milstein) and the general MFMA kernel on 4-row    */
                           /* tiles (Euler, Milstein, SRK); the member is a prologue property of these kernels (their       */
                           /* launch's second grid axis), not a kernel of its own.  A plan that arrives at any other kernel */
                           /* (16-row tiles, wave pairs, the diffusion-net kernels, H = 256, the two-tile kernels) is no    */
                           /* plan: snsde_forward_path == SNSDE_PATH_NONE, the launch is SNSDE_ERR_UNSUPPORTED, and `auto`  */
                           /* does not fall to the generic family.  The workspace holds one prepared block per member:      */
                           /* snsde_workspace_bytes = M x (the plan's floats rounded up to a multiple of four, plus the     */
                           /* 64-float tail of every workspace), so every block starts 16-byte aligned; one prepare launch  */
                           /* fills all of them and SNSDE_FLAG_REUSE_PREPARED skips it as for one model.                    */
                           /* Training through an ensemble is opt-in, SNSDE_FLAG_ENSEMBLE_GRAD; without the flag everything */
                           /* above holds.  With it act_save, stage_save, traj, dW_out and dU_out are accepted by the lean  */
                           /* kernel and the general kernel on 4-row tiles (elementwise diffusions, H <= 128); with these   */
                           /* planes any other plan is SNSDE_PATH_NONE / SNSDE_ERR_UNSUPPORTED.  Every plane is             */
                           /* (.., batch, H), member-major like ys.  snsde_backward_supported is 1 where the adjoint is the */
                           /* general MFMA adjoint on 4-row tiles (Euler / Milstein) or its SRK form, 0 for everything else */
                           /* (kernel = generic / 16-row tiles, wave pairs, diffusion nets, H = 256, the two-tile kernels,  */
                           /* Milstein with noise_option 7, samples > 1, z0_weight, noise_table, kl_column1, the field      */
                           /* variants, bf16 operands): never another kernel, no mode 2.  snsde_solve_backward,             */
                           /* snsde_param_gradients, snsde_backward_with_gradients, their workspace queries and             */
                           /* snsde_save_layout then take the descriptor; grad_params is (M, snsde_param_numel), block m    */
                           /* the sum over member m's own passes x Bm reduction rows.  Every result of member m - states,   */
                           /* saved planes, adjoints, dL/dy0, delta planes, parameter gradients - equals bit for bit that   */
                           /* of the member-alone shard above: each member is planned as its own solve of Bm rows.  The two */
                           /* backward workspaces hold one block per member:                                                */
                           /*   snsde_backward_workspace_bytes        = M x ((the member-alone solve's bytes + 15) & ~15)   */
                           /*   snsde_param_gradients_workspace_bytes = M x ((the member-alone solve's bytes + 15) & ~15)   */
                           /* (a block starts 16-byte aligned).  The adjoint's pack launch and the three launches of the    */
                           /* weight-gradient pass carry the member on a grid axis: no launch per member.                   */
                           /* snsde_coeff_gradients stays SNSDE_ERR_UNSUPPORTED (workspace query 0) for members > 1.        */
                           /* Sample paths of an ensemble are opt-in, SNSDE_FLAG_ENSEMBLE_SAMPLES; without the flag         */
                           /* samples > 1 stays refused as above.  With it and samples = S > 1: `batch` counts all paths of */
                           /* all members, member-major - row r = m Bm + p, Bm = batch / M paths per member, p = b S + s;   */
                           /* `coeffs` is (Bm / S, L-1, 4C), shared, and row r reads coefficient row (r - m Bm) / S;        */
                           /* everything per row stays per row and the Philox counter stays (row_offset + r, ..).           */
                           /* SNSDE_ERR_DIMS also where Bm % S != 0 (and, as for samples alone, row_offset % S or           */
                           /* global_rows % S != 0).  Member m's rows equal, bit for bit, the SAMPLED solve of member m     */
                           /* alone run as a shard: members = 0, samples = S, batch = Bm, params = block m, row_offset +    */
                           /* m Bm, the same global_rows.  Kernels: those that take both options - the lean kernel and the  */
                           /* general kernel on 4-row tiles; workspace sizes are those of `members`.  Training needs        */
                           /* SNSDE_FLAG_ENSEMBLE_SAMPLES | SNSDE_FLAG_ENSEMBLE_GRAD | SNSDE_FLAG_SAMPLE_GRAD together and  */
                           /* is covered exactly where SNSDE_FLAG_ENSEMBLE_GRAD covers the ensemble; each member is planned */
                           /* as its own sampled solve of Bm paths and every result equals that solve's bit for bit.  The   */
                           /* saved planes are per path (memory grows S times).  z0_weight, noise_table, kl_column1,        */
                           /* snsde_eval_fg and snsde_coeff_gradients stay refused.                                         */
                           /* The diffusion-net kernels are opt-in, SNSDE_FLAG_ENSEMBLE_NETS; without the flag a plan that  */
                           /* arrives at them stays no plan, as above.  With it the ensemble also runs on the wave pairs    */
                           /* (SNSDE_FWD_W4: H = 64, Euler / SRK; a pair reads params + m x snsde_param_numel, no workspace */
                           /* block) and on the diffusion-net 4-row tiles (SNSDE_FWD_M4N: SRK, Milstein, Euler at H = 128   */
                           /* or with a wide control path, H = 16 .. 128; the member is the launch's second grid axis and   */
                           /* the prepare launch packs every layer of the plan, the transposed ones of Milstein included,   */
                           /* into each member's block).  The contract, the dimension errors and the workspace rule are     */
                           /* those above.  With SNSDE_FLAG_ENSEMBLE_SAMPLES as well these two kernels take samples = S > 1 */
                           /* of the ensemble (coefficient row (r - m Bm) / S; the member alone is then the ordinary solve  */
                           /* of Bm rows on coefficients replicated S times: plain samples > 1 on one model stays refused   */
                           /* on these kernels).  Still refused under the flag: z0_weight, noise_table, kl_column1, bf16    */
                           /* operands, the field variants, kernel = generic / 16-row tiles, and every training plane, with */
                           /* or without SNSDE_FLAG_ENSEMBLE_GRAD (snsde_backward_supported == 0).                          */
                           /* Training through the wave pairs is opt-in once more, SNSDE_FLAG_ENSEMBLE_NETS_GRAD together   */
                           /* with SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_GRAD; without all three everything above  */
                           /* holds.  With them the training planes are accepted where the plan arrives at SNSDE_FWD_W4,    */
                           /* and snsde_backward_supported is 1 where the adjoint of the member run alone is                */
                           /* SNSDE_REV_W4_FUSED (Euler or SRK; snsde_backward_kernel reports it, snsde_save_layout answers */
                           /* delta_slots == 0: delta_save is not written).  The member is the second grid axis of the      */
                           /* forward, of the adjoint and of the two reduction launches: one launch each for all members.   */
                           /* The contract is the one above: states, saved planes, adjoints, dL/dy0 and block m of          */
                           /* grad_params equal the member-alone shard's bit for bit.  snsde_backward_workspace_bytes = M x */
                           /* ((the member-alone solve's bytes + 15) & ~15) as above - each block holds that member's theta */
                           /* partials and per-tile gradient blocks, laid out as the member alone lays them out;            */
                           /* snsde_workspace_bytes is the ensemble's.  Still 0 / SNSDE_PATH_NONE under the three flags:    */
                           /* the diffusion-net 4-row tiles (Milstein, H = 16 / 32 / 128), samples > 1, bf16 operands, the  */
                           /* field variants, kernel = generic / 4-row / 16-row tiles, z0_weight, noise_table, kl_column1.  */
                           /* Never another kernel, no mode 2.                                                              */
    int64_t  row_offset;  /* global index of local row 0 (batch shards keep the global Philox   */
                           /* stream: counter = (row_offset + row, step >> 2, col, stream),      */
                           /* output element step & 3); the planner sees the local batch unless  */
                           /* `global_rows` (below) is set.  Range: 0 <= row_offset and          */
                           /* row_offset + batch <= 2^32, with or without global_rows:           */
                           /* SNSDE_ERR_DIMS otherwise, from every entry point that validates    */
                           /* the descriptor.  The first counter word is the global row itself,  */
                           /* never the global row modulo 2^32: a call whose rows would reach    */
                           /* 2^32 is refused, it does not re-draw the paths of rows 0 ..        */
    uint64_t seed;         /* Philox key                                                         */
    const float*   params;    /* device, snsde_param_numel floats (members = M > 1: M such blocks) */
    const float*   coeffs;    /* device (B, L-1, 4C) = cat[a, b, two_c, three_d] (members: (B / M, ..)) */
    const float*   step_tab;  /* device (N, SNSDE_STEP_STRIDE)                                   */
    const int32_t* out_step;  /* device (T-1)                                                    */
    const float*   out_w;     /* device (T-1, 2)                                                 */
    const float*   y0;        /* device (B, H)                                                   */
    const float*   dW;        /* device (N, B, H) supplied increments bm(t0,t1), or NULL: Philox */
    float*         ys;        /* device (T, B, H) out; ys[0] = y0                                */
    float*         traj;      /* optional device (N+1, B, H): every solver state                 */
    float*         dW_out;    /* optional device (N, B, H): the increments actually used         */
    const float*   srk_tab;   /* device (N, 4, SNSDE_SRK_STRIDE), method SNSDE_SRK only              */
    const float*   dU;        /* device (N, B, H) supplied space-time Levy integrals I_k0 (SRK with   */
                              /* supplied dW), or NULL: h*(dW/2 + sqrt(h/12) xi), xi from Philox      */
    float*         dU_out;    /* optional device (N, B, H): the I_k0 actually used                    */
    float*         act_save;  /* optional device (N, snsde_act_slots, B, H): per-step activations the MFMA adjoint */
                              /* needs (training mode; see snsde_solve_backward).  Models with the relu activation: */
                              /* the last drift slot (the pre-tanh drift output z; one per pass under SRK) carries, */
                              /* in its low num_hidden_layers mantissa bits, the signs of the step's / pass's        */
                              /* rectified layer outputs (bit k = [slot k > 0] of the same element; through a two-  */
                              /* layer diffusion net under SRK / Milstein also the net's hidden signs, one or two    */
                              /* bits above) - the adjoints' relu masks, so that they do not re-read the activation  */
                              /* planes; z itself is exact to 1e-6 .. 1e-5 relative there                            */
    float*         stage_save;/* SRK training on the MFMA path: optional device (3N + 1, planes, B, H), the input state of */
                              /* every drift pass (act_save / delta_save are then indexed by pass, 3N of them); planes = 1, */
                              /* or 3 with a diffusion net (snsde_save_layout)                                              */
    const uint64_t* seed_dev; /* optional device pointer to the Philox key: read when the kernel starts and used  */
                              /* instead of `seed`, so a captured hipGraph draws fresh increments on every replay */
                              /* (the owner updates the value in-stream between replays).                         */
    const float*   noise_table;/* optional device (N, H): the time-only factor of the diffusion per solver step, supplied by  */
                              /* the caller instead of being evaluated from noise_t (noise_option 12: raw = table[n],     */
                              /* 13: raw = table[n] * y).  Used for fields whose time-only diffusion net is not noise_t.   */
    const int32_t* row_out;   /* optional device (B): per-row output selection (the gather of NeuralSDE.forward,  */
                              /* neuralsde.py:115-116).  When set, ys is (B, H) with ys[b] = the solution at      */
                              /* ts[row_out[b]] (0 <= row_out[b] < n_out), and the backward's grad_ys is (B, H).  */
    const float*   z0_weight; /* optional device (H, C) + z0_bias (H): the wrapper's initial_network.  When set, the   */
    const float*   z0_bias;   /* solve starts from y0 = z0_weight . X(ts[0]) + z0_bias (NeuralSDE._prepare_initial_state, */
                              /* neuralsde.py:63-69) and `y0` is an OUTPUT: the caller passes an uninitialised (B, H)      */
                              /* buffer, the library fills it in the same launch that packs the weights.                   */
    void*          workspace; /* device scratch, >= snsde_workspace_bytes()                      */
    size_t         workspace_bytes;
    /* Path-integral accumulator column (torch-ists LatentSDE.f_aug / g_aug, diff_module/NSDE/latent_sde.py:60-89): when
     * kl_column1 = 1 + c > 0, state column c is NOT driven by the drift net but integrates, with the scheme's own drift
     * weights and no noise,  u(t, y) = 1/2 sum_{j < c} ((f_j(t, y) - (kl_prior_a y_j + kl_prior_b)) / g_j)^2  - the KL rate
     * between the posterior drift f and the linear prior drift theta (mu - y) (a = -theta, b = theta mu) under the shared
     * diagonal diffusion g (the solve's additive noise_table, |g| floored at 1e-7 as the reference's _stable_division).
     * Columns above c must be padding (zero weights).  Field variants on the 4-row-tile kernels only (SNSDE_DRIFT_LINEAR,
     * SNSDE_DIFFUSION_RAW with a noise_table, noise_option 12): Euler / Milstein on the lean kernel, SRK on the SRK variant;
     * the MFMA adjoints carry the accumulator's cotangent back into the drift (snsde_backward_supported == 1).            */
    int32_t        kl_column1;
    float          kl_prior_a;
    float          kl_prior_b;
    int32_t        reserved2;  /* must be 0                                                          */
    /* Rows of the WHOLE problem this call is a batch shard of (rows row_offset .. row_offset + batch - 1 of it), or 0: this call
     * is the whole problem.  When set (>= row_offset + batch, SNSDE_ERR_DIMS otherwise) every choice between kernels whose
     * results are not bit-identical to each other - 16-row / 4-row tiles, the wave-pair kernels, the wave-pair adjoint - is made as
     * for `global_rows` rows on one device, by every entry point that plans (snsde_forward_path, snsde_lean_variant,
     * snsde_backward_supported, snsde_save_layout, the workspace queries, both launches): the shards of a problem then run the
     * kernel the unsharded problem runs and reproduce its states, trajectory, saved planes, per-row adjoints and dL/dy0 bit for
     * bit (parameter gradients: per-shard sums, equal within rounding).  Grids, ragged tails, workspace sizes and the 32-bit
     * save-offset guards stay per shard.  A shard the global plan's kernel cannot run (fewer than 4 rows under a wave-pair plan)
     * is SNSDE_ERR_UNSUPPORTED: never another kernel. */
    int64_t        global_rows;
    /* Monte-Carlo sample paths: S = samples > 1 Brownian paths per input row in one solve (0 or 1: one path per row, today's
     * behaviour).  `batch` is then the number of PATHS of this call; path p (local row p) integrates against input row p / S:
     * coeffs is (batch / S, L-1, 4C), while y0, ys, dW, dU and row_out stay per path, (batch, ...).  The Philox counter stays
     * (row_offset + p, step >> 2, col, stream), so the solve equals, bit for bit, the same descriptor with samples = 0 and every row
     * of coeffs repeated S times - without the S copies in memory.  batch, row_offset (and global_rows where set) must be
     * multiples of S, S >= 0: SNSDE_ERR_DIMS otherwise.  Inference only: act_save, stage_save, traj, dW_out, dU_out or
     * z0_weight (the host materialises y0) is SNSDE_ERR_UNSUPPORTED, as are snsde_eval_fg and every backward entry point
     * (snsde_backward_supported == 0).  Kernels: the lean 4-row-tile kernel (f32, specialised, bf16), the general MFMA kernel
     * (4- and 16-row tiles; Euler, Milstein, SRK) and the generic family.  A plan that arrives at another kernel is no plan:
     * snsde_forward_path == SNSDE_PATH_NONE and the launch is SNSDE_ERR_UNSUPPORTED, never another kernel.
     * snsde_workspace_bytes does not depend on it.
     * Training through the sample paths is opt-in, SNSDE_FLAG_SAMPLE_GRAD; without the flag everything above holds.  With it,
     * act_save, stage_save, traj, dW_out and dU_out are accepted by the lean kernel (general and specialised) and the general MFMA
     * kernel (4- and 16-row tiles; Euler, Milstein, SRK; elementwise diffusions, H <= 128) - the plans snsde_backward_supported
     * answers 1 for; with these planes any other plan is SNSDE_PATH_NONE / SNSDE_ERR_UNSUPPORTED.  Every saved plane is per path, (.., batch, ..), exactly as in the solve
     * with replicated coefficients, so training memory grows S times and only the coefficient side stays at batch / S rows.
     * z0_weight and snsde_eval_fg stay refused.  snsde_backward_supported plans such a descriptor: 1 where the MFMA adjoint with
     * delta planes (snsde_save_layout: delta_slots > 0) takes it; the generic adjoints (mode 2), the wave-pair kernels, the
     * diffusion-net kernels, H = 256, the H = 128 two-tile kernel, the field variants and kl_column1 != 0 are 0, and such a plan
     * is no plan: never another kernel.  snsde_solve_backward, snsde_param_gradients, snsde_backward_with_gradients,
     * snsde_coeff_gradients, their workspace queries and snsde_save_layout then take the descriptor; the adjoints, delta planes and
     * parameter gradients equal those of the replicated solve bit for bit, and grad_coeffs is (batch / S, L-1, 4C): the sum over
     * the S paths of an input row, formed in place (snsde_coeff_gradients).
     * Together with members = M > 1: refused, unless SNSDE_FLAG_ENSEMBLE_SAMPLES opts in (snsde_solve.members, last paragraph:
     * the sample groups then count from each member's first row, and Bm = batch / M must be a multiple of S as well). */
    int32_t        samples;
    int32_t        reserved3;  /* must be 0                                                          */
} snsde_solve;

SNSDE_API size_t snsde_workspace_bytes(const snsde_solve* s);
SNSDE_API int    snsde_solve_forward(const snsde_solve* s, void* hip_stream);
/* Resumable solves: the same solve, drawing its Brownian path from global solver step `step_offset` = n0 on.  Like row_offset and
 * seed, n0 is a coordinate of the random stream, not a plan input: it is no descriptor field, no planning query reads it and the
 * route - the kernel snsde_forward_kernel / snsde_lean_variant name for the descriptor - is the same at every offset.
 * Philox counters: local solver step i of this call draws the normals the library specifies for global step n0 + i - counter
 * (row_offset + row, (n0 + i) >> 2, col, stream), output element (n0 + i) & 3 - for both streams (0: the increment, 1: the normal of
 * the SRK space-time Levy area).  Everything else stays local to the call: step_tab, srk_tab, out_step, out_w, noise_table, supplied
 * dW / dU, traj, dW_out, dU_out and ys are indexed by the local step as in snsde_solve_forward.  With a supplied dW the offset only
 * moves what is still drawn (under SRK nothing: dU is required then).
 * Cutting a solve: cut a solve of N steps at 0 = c_0 < c_1 < .. < c_k = N; chunk j gets rows c_j .. c_{j+1} - 1 of the step table
 * (and of srk_tab), step_offset = c_j, y0 = the state after step c_j - 1, and the same seed, row_offset, global_rows, samples and
 * members.  Every chunk then reproduces the states of the uncut solve bit for bit, on the same kernel.
 * snsde_solve_forward(s, st) is snsde_solve_forward_at(s, 0, st): the same launches, the same bits.
 * SNSDE_ERR_DIMS: step_offset < 0 or step_offset + n_steps > INT32_MAX.  SNSDE_ERR_UNSUPPORTED for step_offset != 0 with z0_weight
 * (a continuation starts from the caller's state, not from X(ts[0])), with or without SNSDE_FLAG_RESUME_GRAD.  traj, dW_out and
 * dU_out are plain outputs, accepted wherever the offset-0 solve of the same descriptor accepts them.  Every check is made before
 * the first launch; all other validation and routing is that of snsde_solve_forward.  Enqueue-only and capturable; the offset is
 * a launch argument and is frozen into a recording.
 * Training planes.  Without SNSDE_FLAG_RESUME_GRAD a continued solve is inference only: SNSDE_ERR_UNSUPPORTED for step_offset != 0
 * with act_save or stage_save, and a descriptor that was run at n0 != 0 must not be handed to a backward entry point.  With the
 * flag, act_save and stage_save are accepted at every offset wherever the offset-0 training forward of the same descriptor accepts
 * them - the same training-mode kernels, which honour n0 at their Philox sites like the inference ones - and the chunk is
 * differentiated by the _at form of a backward entry point with the chunk's own step_offset: snsde_solve_backward_at,
 * snsde_backward_with_gradients_at.  The adjoints that regenerate Philox increments in-kernel (Euler / Milstein with a host key
 * and neither dW_out nor a supplied dW) then draw global step n0 + n for local step n - block (n0 + n) >> 2, element (n0 + n) & 3,
 * n0 a uniform kernel argument - bit for bit the product the forward formed; the adjoints that read dW_out or a supplied dW (SRK,
 * the diffusion-net tiles, mode 2, a device-resident key) take the offset and need nothing from it.  snsde_param_gradients and
 * snsde_coeff_gradients read no increments and have no _at form.  Cut a training solve as above with grad_ys of chunk j carrying,
 * in its last output row, the chunk j + 1 adjoint adj[0]: dL/dy0 follows the adjoint recursion of the uncut solve, and the
 * parameter and coefficient gradients of the uncut solve are the sums of the chunks'. */
SNSDE_API int    snsde_solve_forward_at(const snsde_solve* s, int64_t step_offset, void* hip_stream);
/* The initial state of a solve with z0_weight / z0_bias as a launch of its own: y0 (B, H, an OUTPUT as there) = z0_weight .
 * X(ts[0]) + z0_bias, through the device code the forward's prepare launch runs - the same bits.  For callers that need the state
 * a fused z0_weight solve would start from where the solve itself cannot form it (a model ensemble takes the caller's y0 and
 * refuses z0_weight: each member's rows are filled by one such call).  Reads model.hidden_channels / input_channels, batch, knots,
 * coeffs (batch, L-1, 4C), step_tab (row 0), z0_weight, z0_bias and y0 only.  Enqueue-only, no workspace, capturable. */
SNSDE_API int    snsde_initial_state(const snsde_solve* s, void* hip_stream);

/* ---- backward of the solve (discretise-then-optimise adjoint of the fixed-step scheme) ------
 * Replaces autograd THROUGH the unrolled solver loop (`loss.backward()` in
 * benchmark_classification/common_sde.py:160, ~25 autograd nodes per solver step): given dL/d ys it runs the adjoint
 * recursion of the scheme (Euler: a_n = a_{n+1} + h (df/dy)^T a_{n+1} + (dg/dy)^T (a_{n+1} * dW_n); Milstein and SRID2: the
 * reverse of their step formulas) backwards over the saved trajectory and writes EVERY a_n (adj[0] = dL/dy0).
 * snsde_backward_supported:
 *   1 = MFMA adjoint kernels: forward on the MFMA path with traj (+ dW_out unless the increments are supplied or Philox ones
 *       can be regenerated; + dU_out, stage_save for SRK) and act_save; Euler, Milstein and SRK, for the elementwise diffusions
 *       AND through the diffusion nets (noise_option 14/15/18/19; Milstein through a two-layer net at H = 128 and the nets at
 *       H = 256 excepted: mode 2); fills delta_save, and snsde_param_gradients then forms every parameter gradient ON THE DEVICE
 *       (split-R MFMA weight-gradient GEMMs over the saved activations / deltas, diffusion-side reductions, the folded
 *       first layer's algebra) in the flat layout of `params`;
 *   2 = generic adjoint kernels (forward on any kernel; traj + dW_out (+ dU_out for SRK) only; Euler, Milstein and SRK, any
 *       dims within the LDS budget, every noise_option (Milstein: all but 7); delta_save must be NULL): adjoints only, the
 *       host layer takes the parameter gradients from one batched evaluation of the step function;
 *   0 = none. */
typedef struct snsde_backward {
    uint32_t     struct_size;/* = sizeof(snsde_backward)                                                            */
    snsde_solve  fwd;        /* the forward descriptor (traj, dW_out, act_save filled by the forward)      */
    const float* grad_ys;    /* device (T, B, H): dL/d ys                                                 */
    float*       adj;        /* device (N+1, B, H) out: adjoint of every solver state                     */
    float*       delta_save; /* optional device (N, snsde_act_slots, B, H) out: per step, slot 0 = dL/d zout and */
                             /* slot g = dL/d(pre-activation of hidden layer slots-1-g): the left factors of    */
                             /* the weight-gradient GEMMs  dW_layer = sum delta^T . layer_input                  */
    void*        workspace;  /* device scratch >= snsde_backward_workspace_bytes (separate from fwd's)    */
    size_t       workspace_bytes;
    float*       grad_noise_table; /* snsde_param_gradients with fwd.noise_table set: optional device (N, H) out,      */
                             /* dL/d noise_table (the caller back-propagates it through whatever produced the table) */
    int32_t      flags;      /* SNSDE_BWD_ADJ0_ONLY: `adj` is (B, H) and receives dL/dy0 only - the MFMA adjoint kernels   */
                             /* (mode 1) need no a_n in memory, except Milstein through a diffusion net, whose second-    */
                             /* order weight-gradient jobs read them (there and in mode 2 the flag is refused: ERR_OPTION) */
    int32_t      reserved;
} snsde_backward;
enum { SNSDE_BWD_ADJ0_ONLY = 1 };

SNSDE_API int    snsde_act_slots(const snsde_model* m);             /* activation tensors saved per step, or <0: layer outputs (first, hidden.., */
                                                          /* pre-tanh drift) [+ diffusion-net slots]; models with a smooth activation  */
                                                          /* (SNSDE_ACT_LIPSWISH / SILU) also save every pre-activation (NL more slots,  */
                                                          /* + the hidden pre-activation of a two-layer diffusion net, the last slot)   */
SNSDE_API int    snsde_save_layout(const snsde_solve* s, int32_t* act_slots, int32_t* stage_planes, int32_t* delta_slots);
                                                          /* training-mode buffers of THIS solve (model + method): act_save /     */
                                                          /* delta_save are (passes, act_slots, B, H), stage_save (passes + 1,     */
                                                          /* stage_planes, B, H); passes = N (3N for SRK).  SRK through a          */
                                                          /* diffusion net (noise_option 14/15/18/19) saves a second set of net    */
                                                          /* slots (the step's fourth diffusion evaluation) and three stage planes */
                                                          /* (drift input H0 | diffusion input H1 | H1 of the fourth evaluation);  */
                                                          /* delta_save is (passes, delta_slots, B, H): act_slots, plus the tangent */
                                                          /* factors of Milstein through a diffusion net; delta_slots == 0: the      */
                                                          /* adjoint of this solve accumulates the weight gradients itself (Euler /  */
                                                          /* SRK at H = 64 with a diffusion net: per-tile sums in the backward       */
                                                          /* workspace), delta_save is not written and may be NULL                   */
SNSDE_API int    snsde_backward_supported(const snsde_solve* s);    /* 1 / 2 / 0, see above; bf16 operands: 0, or 1 under */
                                                                    /* SNSDE_FLAG_BF16_GRAD where it covers the solve;    */
                                                                    /* members > 1: 0, or under SNSDE_FLAG_ENSEMBLE_GRAD  */
                                                                    /* 1 where the general 4-row-tile adjoint takes it,   */
                                                                    /* with SNSDE_FLAG_ENSEMBLE_NETS and _NETS_GRAD as    */
                                                                    /* well 1 where the wave-pair adjoint takes it        */
SNSDE_API size_t snsde_backward_workspace_bytes(const snsde_backward* b);
/* INVARIANT between forward and backward (mode 1): `fwd.workspace` is untouched AND `fwd.params` holds the values the forward ran
 * with.  The adjoint re-packs its transposed weights from the CURRENT params, but takes the folded first-layer product
 * emb . linear_in (input_option 2 / 4 / 6) from the forward's workspace: an in-place parameter update between the two calls, or a
 * second forward through the same workspace, mixes old and new weights without an error.  (torchsde.sdeint keeps both: the
 * autograd node owns the workspace and runs before the optimizer step.)                                                        */
/* fwd.members = M > 1 under SNSDE_FLAG_ENSEMBLE_GRAD: grad_ys, adj and delta_save hold the rows of all members like ys; member m's
 * tiles read block m of fwd.params, of fwd.workspace and of b->workspace.  SNSDE_BWD_ADJ0_ONLY, row_out and supplied dW / dU as
 * for one model.  Without the flag: SNSDE_ERR_UNSUPPORTED.  On the wave pairs (SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_GRAD |
 * SNSDE_FLAG_ENSEMBLE_NETS_GRAD): no delta planes; member m's pairs leave their theta partials and gradient blocks in block m of
 * b->workspace. */
SNSDE_API int    snsde_solve_backward(const snsde_backward* b, void* hip_stream);
/* The backward of a chunk that snsde_solve_forward_at ran at `step_offset` (its last paragraph): the same call, the adjoint's
 * regenerated increments those of global steps step_offset + n.  snsde_solve_backward(b, st) is snsde_solve_backward_at(b, 0, st):
 * the same launches, the same bits.  SNSDE_ERR_DIMS: step_offset < 0 or step_offset + fwd.n_steps > INT32_MAX.
 * SNSDE_ERR_UNSUPPORTED: step_offset != 0 and b->fwd.flags lacks SNSDE_FLAG_RESUME_GRAD.  Both after the descriptor's own checks,
 * before any launch. */
SNSDE_API int    snsde_solve_backward_at(const snsde_backward* b, int64_t step_offset, void* hip_stream);

/* Parameter gradients of the fused solve (mode 1 = MFMA path only): after snsde_solve_forward (traj, dW_out, act_save
 * kept; fwd.workspace untouched since) and snsde_solve_backward (adj, delta_save; b->workspace still the buffer that
 * call used — it holds the adjoint kernel's per-workgroup diffusion-side sums), writes dL/d params into
 * grad_params (device, snsde_param_numel floats, same flat layout as `params`, overwritten) — what autograd
 * accumulates through the unrolled loop (benchmark_classification/common_sde.py:158-160): split-R MFMA GEMMs
 * sum_r delta^T . input with per-workgroup partials and one deterministic reduction, the elementwise diffusion
 * reductions (theta, the time-only noise MLP; Euler and Milstein) and the first-layer/emb algebra.
 * `b` is the descriptor snsde_solve_backward ran with, workspace included: the adjoint's workspace is an INPUT here (its
 * per-workgroup diffusion-side sums; with delta_slots == 0 the per-tile weight-gradient blocks) - SNSDE_ERR_NULL without it,
 * SNSDE_ERR_WORKSPACE when workspace_bytes < snsde_backward_workspace_bytes(b).
 * fwd.members = M > 1 under SNSDE_FLAG_ENSEMBLE_GRAD: grad_params is (M, snsde_param_numel); block m sums member m's rows only, in
 * the order the member-alone solve sums them (bit-equal), all members in the same launches (the wave pairs under
 * SNSDE_FLAG_ENSEMBLE_NETS_GRAD: one zero fill and the two reduction launches, the member on their third grid axis). */
SNSDE_API size_t snsde_param_gradients_workspace_bytes(const snsde_backward* b);
SNSDE_API int    snsde_param_gradients(const snsde_backward* b, float* grad_params, void* workspace, size_t workspace_bytes,
                             void* hip_stream);

/* snsde_solve_backward followed by snsde_param_gradients as ONE call (mode 1 solves only; same arguments, same results bit for
 * bit): one transition from the host language and one validation instead of two, the launches back to back on the stream.
 * Enqueue-only and capturable like the two calls it replaces; returns SNSDE_ERR_UNSUPPORTED where snsde_backward_supported()
 * != 1 (the caller then uses the separate calls).  A model ensemble under SNSDE_FLAG_ENSEMBLE_GRAD (on the wave pairs: with
 * SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_NETS_GRAD): as the two calls.                                                    */
SNSDE_API int snsde_backward_with_gradients(const snsde_backward* b, float* grad_params, void* pg_workspace, size_t pg_workspace_bytes,
                                            void* hip_stream);
/* ... of a chunk run at `step_offset`: snsde_solve_backward_at followed by snsde_param_gradients (which reads no increments).  The
 * name above is this call at offset 0; the offset's errors as for snsde_solve_backward_at. */
SNSDE_API int snsde_backward_with_gradients_at(const snsde_backward* b, float* grad_params, void* pg_workspace, size_t pg_workspace_bytes,
                                               int64_t step_offset, void* hip_stream);

/* Gradient of the fused solve with respect to the control path, dL/d coeffs (mode 1 = MFMA path only), from what the adjoint left
 * in HBM.  X(t) enters the drift's first layer only, and linearly: with delta_p (B, H) = dL/d(pre-activation of the drift's first
 * rectified layer) at drift pass p (delta_save slot num_hidden_layers, the plane the weight-gradient pass reads for the folded
 * first layer; passes = N, SRK: the three drift stages of every step), evaluated on spline interval k_p at offset r_p (step_tab
 * columns 5 / 4; SRK: the srk_tab slot of the pass's drift stage), and
 *     M (H, C) = emb.weight[:, H:] . initial_network.weight  (input_option 2 / 4 / 6),  initial_network.weight  (input_option 0)
 * the call writes
 *     grad_coeffs[b, k, j C + c] = sum_{p : k_p = k} phi_j(r_p) (delta_p M)[b, c],   phi = (1, r, r^2 / 2, r^3 / 3)
 * for the blocks (a, b, two_c, three_d) - the derivatives of a + (b + (two_c / 2 + three_d r / 3) r) r.  The diffusion never
 * reads X.  Intervals no pass falls into receive exactly 0; grad_coeffs (B, L-1, 4C) is overwritten.
 * `b` is the descriptor snsde_solve_backward (or snsde_backward_with_gradients) ran with; delta_save is filled.  Enqueue-only and
 * capturable: no allocation, no synchronisation.  Deterministic: no floating-point atomics, every (b, k, j, c) is summed by one
 * owner in ascending pass order, so two runs are bit-equal; a row's result depends on that row's planes alone, so batch shards
 * (row_offset / global_rows) reproduce the rows of the whole bit for bit.
 * input_option 1 / 3 / 5 (the drift does not read X): grad_coeffs is zero-filled, SNSDE_OK.  SNSDE_ERR_UNSUPPORTED: a solve
 * whose adjoint leaves no delta planes (snsde_save_layout: delta_slots == 0, the H = 64 wave-pair adjoints), mode 2 or 0,
 * delta_save == NULL, fwd.members > 1 (with or without SNSDE_FLAG_ENSEMBLE_GRAD), fwd.samples > 1 without SNSDE_FLAG_SAMPLE_GRAD, fwd.kl_column1 != 0, the field variants, a supplied noise_table and
 * SNSDE_FLAG_BF16_OPERANDS (also under SNSDE_FLAG_BF16_GRAD: the rounded folded control-path weights are not formed here).  SNSDE_ERR_NULL /
 * SNSDE_ERR_WORKSPACE as elsewhere; every check happens before the first launch.  The dependence of y0 on coeffs through a fused
 * z0_weight is not part of this gradient (the host materialises y0 with tensor ops when coeffs require a gradient).
 * fwd.samples = S > 1 under SNSDE_FLAG_SAMPLE_GRAD: delta_save holds `batch` paths and grad_coeffs is (batch / S, L-1, 4C),
 *     grad_coeffs[b, k, j C + c] = sum_{p : k_p = k} sum_{s < S} phi_j(r_p) (delta_p M)[b S + s, c]
 * - one owner per element that walks the passes in ascending order and, inside a pass, the paths s = 0 .. S-1 in order.  A path
 * whose delta planes are zero adds exact zeros; a row's result depends on the planes of its own S paths alone, so a shard of whole
 * groups reproduces its rows of the whole bit for bit.  The workspace holds v for `batch` paths. */
SNSDE_API size_t snsde_coeff_gradients_workspace_bytes(const snsde_backward* b);
SNSDE_API int    snsde_coeff_gradients(const snsde_backward* b, float* grad_coeffs /* (B, L-1, 4C), overwritten */,
                                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- cubic spline evaluation (A10) -----------------------------------------------------------
 * out[b, c] = a + (b + (0.5*two_c + three_d*frac/3)*frac)*frac   on interval `index`
 * (derivative != 0: b + (two_c + three_d*frac)*frac), operation order as
 * controldiffeq/interpolate.py:270-283 (bit-exact with the CPU reference).  Every element of out
 * (batch, channels) is written and nothing else; coeffs is only read; no workspace, no alignment
 * beyond that of a float.                                                                       */
SNSDE_API int snsde_spline_evaluate(const float* coeffs, int32_t batch, int32_t knots, int32_t channels,
                          int32_t index, float frac, int32_t derivative, float* out, void* hip_stream);

/* ---- spline coefficient construction (A11 / A12; offline preprocessing in the reference) ------------
 * natural: controldiffeq.natural_cubic_spline_coeffs (interpolate.py:161-228) incl. its missing-value handling;
 * hermite: torchcde.hermite_cubic_coefficients_with_backward_differences (datasets/common.py:82-84).
 * times (L) and X (B, L, C) device float32, NaN = missing; coeffs (B, L-1, 4C) = cat[a, b, two_c, three_d] out.
 * Every element of coeffs is written - a series without an observation included - and no byte outside it but the workspace of
 * the natural construction, which is written before it is read (its contents on entry do not matter).  times and X are only read.
 * The pointers need the alignment of a float and no more. */
SNSDE_API size_t snsde_spline_workspace_bytes(int32_t batch, int32_t knots, int32_t channels);
SNSDE_API int snsde_natural_cubic_coeffs(const float* times, const float* X, int32_t batch, int32_t knots, int32_t channels,
                               float* coeffs, void* workspace, size_t workspace_bytes, void* hip_stream);
SNSDE_API int snsde_hermite_coeffs(const float* times, const float* X, int32_t batch, int32_t knots, int32_t channels,
                         float* coeffs, void* hip_stream);

/* Adjoints of the two constructions: grad_X (B, L, C) = J^T grad_coeffs, J the (linear) map X -> coeffs.  The knot compaction,
 * the tridiagonal matrix, the end imputation and the fill weights depend on `times` and on WHICH entries of X are NaN only, so X is
 * read for its mask and nothing of the forward is needed.  Every entry of grad_X is written: missing entries and series without an
 * observation get exactly 0.  One lane per series, a fixed operation order, no atomics: bit-equal from run to run and independent
 * of the batch a row sits in.  Enqueue-only on hip_stream.  SNSDE_ERR_NULL / SNSDE_ERR_DIMS / SNSDE_ERR_WORKSPACE as the
 * constructions; every check happens before the launch.  The Hermite adjoint needs no workspace. */
SNSDE_API size_t snsde_spline_backward_workspace_bytes(int32_t batch, int32_t knots, int32_t channels);
SNSDE_API int snsde_natural_cubic_coeffs_backward(const float* times, const float* X, const float* grad_coeffs,
                                        int32_t batch, int32_t knots, int32_t channels,
                                        float* grad_X, void* workspace, size_t workspace_bytes, void* hip_stream);
SNSDE_API int snsde_hermite_coeffs_backward(const float* times, const float* X, const float* grad_coeffs,
                                  int32_t batch, int32_t knots, int32_t channels,
                                  float* grad_X, void* hip_stream);

/* vector-field probe: one evaluation of f(t,y) and g(t,y) (neuralsde.py:295-307) through the same
 * device code the solver uses.  `step_row` = one step_tab row (device, SNSDE_STEP_STRIDE floats)
 * describing t; y, f_out, g_out are device (B, H).  Uses s->model/batch/knots/params/coeffs/
 * workspace only.                                                                             */
SNSDE_API int snsde_eval_fg(const snsde_solve* s, const float* step_row, const float* y, float* f_out,
                  float* g_out, void* hip_stream);

/* Kernel family a forward solve of this descriptor runs on (host-side query, no device access): the coverage table in
 * profiles/ is generated from it.                                                                                  */
enum { SNSDE_PATH_NONE = 0,          /* no kernel: snsde_solve_forward returns SNSDE_ERR_UNSUPPORTED                 */
       SNSDE_PATH_GENERIC = 1,       /* generic kernel family (every option, any dims; one wave per row group)      */
       SNSDE_PATH_MFMA_M16 = 2,      /* MFMA, 16-row tiles                                                          */
       SNSDE_PATH_MFMA_M4 = 3,       /* MFMA, 4-row tiles, general kernel                                           */
       SNSDE_PATH_LEAN = 4,          /* MFMA, 4-row tiles, lean kernel (register-resident weights, H = 32/64/128)    */
       SNSDE_PATH_LEAN_STREAMED = 5, /* MFMA, 4-row tiles, lean kernel with L2 -> LDS streamed weights (H = 256)     */
       SNSDE_PATH_GENERIC_SRK = 6,   /* SRK on the generic family                                                   */
       SNSDE_PATH_MFMA_SRK = 7,      /* SRK on the MFMA 4-row tiles                                                 */
       SNSDE_PATH_MFMA_W4 = 8,       /* MFMA, 4 rows per wave pair (csrc/snsde_w4_kernel.h: H = 64, diffusion nets, Euler / SRK) */
       SNSDE_PATH_LEAN_BF16 = 9 };   /* the lean kernel with bf16 MFMA operands (SNSDE_FLAG_BF16_OPERANDS, H = 64 / 128)      */
SNSDE_API int snsde_forward_path(const snsde_solve* s);
/* Host-only query next to snsde_forward_path: which instantiation of the lean kernel (SNSDE_PATH_LEAN, one 4-row tile per
 * workgroup) snsde_solve_forward would launch.  SNSDE_LEAN_GENERAL = the instantiation that tests the field's options at run
 * time; SNSDE_LEAN_SPECIALISED = one compiled for exactly this field's options (csrc/snsde_m4_kernel.h: CfgSpec), the same
 * results bit for bit.  SNSDE_LEAN_NONE when the forward runs on another kernel. */
enum { SNSDE_LEAN_NONE = 0, SNSDE_LEAN_GENERAL = 1, SNSDE_LEAN_SPECIALISED = 2 };
SNSDE_API int snsde_lean_variant(const snsde_solve* s);
/* Host-only queries next to snsde_forward_path / snsde_backward_supported: the exact kernel the plan of this descriptor names, one
 * value per kernel the launchers dispatch on (csrc/snsde_mfma_kernels.h: FwdKernel / RevKernel) - the families above fold several
 * of them into one value.  Both read the route the launches dispatch on (route_forward / route_backward) and re-derive nothing, so
 * they see what a launch sees: the training-mode pointers, the supplied increments and the flags of THIS descriptor.
 * snsde_forward_kernel: nhid / kuxt (each may be NULL) receive the plan's hidden-layer count and its 16-wide k-blocks of
 * [X(t) | sin t, cos t] on an MFMA route - the keys of the two-tile kernels' instantiation lists - and -1 otherwise.
 * snsde_backward_kernel: SNSDE_REV_NONE exactly where snsde_backward_supported is 0, SNSDE_REV_GENERIC exactly where it is 2. */
enum { SNSDE_FWD_NONE = 0,                /* no kernel (SNSDE_PATH_NONE)                                                    */
       SNSDE_FWD_GENERIC = 1,             /* generic family, Euler / Milstein (SNSDE_PATH_GENERIC)                          */
       SNSDE_FWD_GENERIC_SRK = 2,         /* generic family, SRK (SNSDE_PATH_GENERIC_SRK)                                   */
       SNSDE_FWD_W4 = 3,                  /* wave pairs (csrc/snsde_w4_kernel.h)                                            */
       SNSDE_FWD_M4N = 4,                 /* diffusion-net kernel on 4-row tiles (csrc/snsde_m4n_kernel.h)                  */
       SNSDE_FWD_LEAN = 5,                /* lean kernel, one tile per workgroup (csrc/snsde_m4_kernel.h)                   */
       SNSDE_FWD_LEAN_TWO_TILE_H128 = 6,  /* H = 128, two tiles per wave (csrc/snsde_m4t_kernel.h; SNSDE_FLAG_TWO_TILE)     */
       SNSDE_FWD_LEAN_TWO_TILE_H256 = 7,  /* H = 256, two tiles per wave (csrc/snsde_m4s2_kernel.h)                         */
       SNSDE_FWD_LEAN_STREAMED_H256 = 8,  /* H = 256, fully streamed weights (csrc/snsde_m4s_kernel.h)                      */
       SNSDE_FWD_GENERAL_M4 = 9,          /* general MFMA kernel, 4-row tiles (its SRK variant included)                    */
       SNSDE_FWD_GENERAL_M16 = 10,        /* general MFMA kernel, 16-row tiles (its SRK variant included)                   */
       SNSDE_FWD_LEAN_BF16 = 11 };        /* lean kernel with bf16 MFMA operands (csrc/snsde_m4b_kernel.h)                  */
SNSDE_API int snsde_forward_kernel(const snsde_solve* s, int32_t* nhid, int32_t* kuxt);
enum { SNSDE_REV_NONE = 0,                /* no fused backward (mode 0)                                                     */
       SNSDE_REV_GENERIC = 1,             /* generic adjoint kernels (mode 2)                                               */
       SNSDE_REV_W4_FUSED = 2,            /* wave-pair adjoint with the weight gradients inside: delta_slots == 0           */
       SNSDE_REV_M4N_SRK = 3,             /* SRK through a diffusion net (csrc/snsde_m4n_rev_kernel.h)                      */
       SNSDE_REV_M4N_MILSTEIN = 4,        /* Milstein through a diffusion net (csrc/snsde_m4n_mil_rev_kernel.h)             */
       SNSDE_REV_GENERAL_SRK = 5,         /* SRK adjoint of the general kernel                                              */
       SNSDE_REV_TWO_TILE_H256 = 6,       /* H = 256, two tiles per wave (csrc/snsde_m4s2_rev_kernel.h)                     */
       SNSDE_REV_GENERAL = 7 };           /* Euler / Milstein adjoint of the general kernel, 4- or 16-row tiles             */
SNSDE_API int snsde_backward_kernel(const snsde_solve* s);

/* Readout head of the wrappers in one launch (inference; replaces the 4-5 tensor ops of `self.linear(z)`,
 * benchmark_classification/models_sde/neuralsde.py:59-61,119; benchmark_forecasting/models_sde/neuralsde.py:186; torch_ists
 * nsde_model.py):  out = W2 relu(bn(W1 act(x) + b1)) + b2  with act = tanh when input_tanh else identity and bn the
 * BatchNorm1d inference transform (v - mean) / sqrt(var + eps) * weight + bias when bn_mean is set.  All pointers device,
 * fp32, row-major contiguous; nn.Linear layout (out_features, in_features).                                              */
typedef struct snsde_head {
    uint32_t struct_size;    /* = sizeof(snsde_head)                                  */
    int32_t rows, in_features, hidden, out_features;
    int32_t input_tanh;
    float   bn_eps;
    const float* x;          /* (rows, in_features)                                   */
    const float* w1;         /* (hidden, in_features)                                 */
    const float* b1;         /* (hidden) or NULL                                      */
    const float* bn_mean;    /* (hidden) running mean, or NULL: no normalisation      */
    const float* bn_var;     /* (hidden) running variance (with bn_mean)              */
    const float* bn_weight;  /* (hidden) or NULL                                      */
    const float* bn_bias;    /* (hidden) or NULL                                      */
    const float* w2;         /* (out_features, hidden)                                */
    const float* b2;         /* (out_features) or NULL                                */
    float*       out;        /* (rows, out_features): every element is written, nothing else is; no workspace */
} snsde_head;
SNSDE_API int snsde_readout_head(const snsde_head* h, void* hip_stream);

/* ---- composed parameter blocks (tutorial-style fields) ---------------------------------------------------------
 * The tutorial notebooks' fields (cell 7 of the tutorial notebooks: linear_in / emb / f_net / linear_out, NeuralSDEFunc's f_net / g_net on
 * [t, y]) map onto the Diffusion_model parameter block by multiplying adjacent affine maps out: W' = W_outer W_inner,
 * b' = W_outer b_inner + b_outer.  These two calls build the block from the field's own tensors and carry the block's gradient back
 * to them, ONE launch each (in torch the same is ~25 + ~35 small launches per training step, which is what bounded that step).
 * A job writes one (weight, bias) pair of the block:
 *   w_outer == NULL : copy         W' = W_inner (R x Cin), b' = b_inner
 *   else            : composition  W' = W_outer (R x K) . W_inner (K x Cin),  b' = W_outer b_inner + b_outer
 * zero_col >= 0 inserts a zero column at that index of W' (the field's [t, y] columns -> the block's [t, 0, y]).
 * dst_w / dst_b: float offsets into `dst` (snsde_param_info); the caller zero-fills what no job writes.
 * The backward reads grad_dst at the same offsets and writes dL/d(each source tensor) at g_* float offsets of `grad_src`
 * (-1: not wanted).  All pointers device, fp32, row-major contiguous; at most SNSDE_MAX_AFFINE_JOBS jobs per call.
 * What a call writes: the forward, per job, the R x (Cin + 1 with a zero column, else Cin) floats at dst_w and the R floats at dst_b,
 * and no other float of dst; the backward, per job and wanted offset, g_w_outer: R K, g_b_outer: R, g_w_inner: K Cin, g_b_inner: K
 * floats (a copy job: g_w_inner: R Cin, g_b_inner: R) and no other float of grad_src - the caller zero-fills that one too.  No
 * workspace; the sources and grad_dst are only read. */
#define SNSDE_MAX_AFFINE_JOBS 12
typedef struct snsde_affine_job {
    const float* w_outer;    /* (R, K) or NULL                                  */
    const float* b_outer;    /* (R) or NULL (only with w_outer)                 */
    const float* w_inner;    /* (K, Cin); copy jobs: (R, Cin)                   */
    const float* b_inner;    /* (K) (copy jobs: (R)) or NULL: b' = b_outer / 0  */
    int32_t R, K, Cin;       /* copy jobs: K ignored                            */
    int32_t zero_col;        /* -1: none                                        */
    int64_t dst_w, dst_b;    /* into dst / grad_dst                             */
    int64_t g_w_outer, g_b_outer, g_w_inner, g_b_inner;   /* into grad_src (backward only; -1: skip) */
} snsde_affine_job;
SNSDE_API int snsde_affine_compose(const snsde_affine_job* jobs, int32_t n_jobs, float* dst, void* hip_stream);
SNSDE_API int snsde_affine_compose_backward(const snsde_affine_job* jobs, int32_t n_jobs, const float* grad_dst, float* grad_src,
                                            void* hip_stream);

/* ---- statistics over sample paths ------------------------------------------------------------
 * ys viewed as (groups, samples, width) - the T leading planes of a (T, B S, H) result of a solve with `samples` = S fold
 * into groups = T B - reduced over the sample axis: mean (groups, width) and, where var != NULL, the unbiased variance
 * (groups, width; / (S - 1), samples < 2 is then SNSDE_ERR_DIMS).  Every element of mean and (where given) var is written and
 * nothing else; ys is only read.  Enqueue-only, no workspace, capturable.  Deterministic:
 * one lane per output element walks s = 0 .. S-1 in order, twice (the sum, then the squared deviations from the mean).
 * All pointers device, fp32, contiguous. */
SNSDE_API int snsde_sample_stats(const float* ys, int64_t groups, int32_t samples, int32_t width, float* mean, float* var,
                                 void* hip_stream);

/* Adjoint of snsde_sample_stats: with grad_mean and (optionally, NULL = none) grad_var, each (groups, width), the ys the
 * statistics were formed from and their mean,
 *     grad_ys[g, s, w] = grad_mean[g, w] / S + grad_var[g, w] * 2 (ys[g, s, w] - mean[g, w]) / (S - 1)
 * (grad_var != NULL with samples < 2 is SNSDE_ERR_DIMS; `mean` is read only with grad_var).  One lane per (g, w) - or four adjacent
 * w - walks s in order; every element of grad_ys is written.  Enqueue-only, no workspace, capturable, deterministic. */
SNSDE_API int snsde_sample_stats_backward(const float* grad_mean, const float* grad_var, const float* ys, const float* mean,
                                          int64_t groups, int32_t samples, int32_t width, float* grad_ys, void* hip_stream);

/* ---- statistics over the sample paths of a model ensemble --------------------------------------
 * ys viewed as (outer, members, groups, samples, width) = (outer, M, G, S, W): a (T, M, B S, H) result of a solve with
 * members = M and samples = S under SNSDE_FLAG_ENSEMBLE_SAMPLES (outer = T, groups = B), or a stacked (M, B S, out) readout
 * (outer = 1).  Outputs (outer, groups, width), each optional (NULL = not wanted).  Per member, exactly as snsde_sample_stats
 * walks them (the same bits):
 *     mean_m = (sum_s x) / S, s ascending;      var_m = (sum_s fmaf(d, d, .)) / (S - 1), d = x - mean_m
 * and across members, m ascending:
 *     mean    = (sum_m mean_m) / M
 *     within  = (sum_m var_m) / M                         the aleatoric part (spread of the noise)
 *     between = (sum_m fmaf(e, e, .)) / (M - 1), e = mean_m - mean      the epistemic part (spread between the models)
 * within + between is the law-of-total-variance estimate of the predictive variance.  `within` with samples < 2 or `between`
 * with members < 2 is SNSDE_ERR_DIMS.  One lane per output element (four adjacent ones with 16-byte accesses where width % 4
 * == 0 and the pointers are 16-byte aligned); no atomics, no dependence on the grid: the same bits on every launch.
 * Every element of each output given is written and nothing else; ys is only read.
 * Enqueue-only, no workspace, capturable.  All pointers device, fp32, contiguous. */
SNSDE_API int snsde_ensemble_stats(const float* ys, int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                   float* mean, float* within, float* between, void* hip_stream);

/* Adjoint of snsde_ensemble_stats: grad_mean, grad_within, grad_between are (outer, groups, width), each may be NULL (none),
 *     grad_ys[o, m, g, s, w] = grad_mean / (M S) + grad_within 2 (x - mean_m) / ((S - 1) M) + grad_between 2 (mean_m - mean) / ((M - 1) S)
 * with the member means recomputed from ys in the forward's order (ys is read only with grad_within or grad_between; the
 * deviations sum to zero, so the terms through the means of the means vanish).  The same lane-per-element ownership; every
 * element of grad_ys is written.  grad_within with samples < 2 or grad_between with members < 2 is SNSDE_ERR_DIMS. */
SNSDE_API int snsde_ensemble_stats_backward(const float* grad_mean, const float* grad_within, const float* grad_between, const float* ys,
                                            int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                            float* grad_ys, void* hip_stream);

/* ---- scores of sample paths against an observation ---------------------------------------------
 * ys viewed as (outer, members, groups, samples, width) = (outer, M, G, S, W) as above (a sampled solve: members = 1, its T B
 * (time, row) pairs fold into groups).  The members axis is addressing only (member stride G S W): the pooled sample set of an
 * output element (o, g, w) is x_n, n = m S + s, N = M S of them - the predictive mixture whose variance snsde_ensemble_stats
 * splits - and a pooled call gives the bits of the members = 1 call on the permuted (outer G, M S, W) tensor.
 * target y is (outer, groups, width).  With d_n = x_n - y, the strict counts c_n = #{j : x_j < x_n} - #{j : x_j > x_n} (ties
 * contribute 0, sum_n c_n = 0) and D = N - 1 (fair != 0: the unbiased estimator; N < 2 is then SNSDE_ERR_DIMS) or D = N,
 *     crps = (sum_n |d_n|) / N - (sum_n c_n d_n) / (N D)            = mean |x - y| - sum_ij |x_i - x_j| / (2 N D)
 *     rank = #{n : x_n < y},  ties = #{n : x_n == y}                (outer, groups, width) as float; each optional, NULL = not wanted
 * One workgroup of four waves stages the (N, 64-column) slab of a group in LDS (N * 256 bytes: N > 256 is SNSDE_ERR_DIMS) and
 * each lane walks its own column; wave k owns the quarter n in [k N / 4, (k + 1) N / 4).  Summation order: the two sums run n
 * ascending inside a quarter (sum += |d_n|; sum = fmaf(c_n, d_n, sum)), the four quarter sums are added k ascending, then one
 * division each and the subtraction.  No atomics, no dependence on the grid: the same bits on every launch.  Enqueue-only, no
 * workspace, capturable.  All pointers device, fp32, contiguous.  SNSDE_ERR_NULL: ys, target or crps NULL.  SNSDE_ERR_DIMS:
 * a non-positive extent, N > 256, fair with N < 2, an element count beyond 63 bits.
 * What the score calls write (snsde_sample_crps, _quantiles, _energy and their adjoints): every element of every output given -
 * crps, rank, ties; out; energy; grad_ys, grad_target - whatever it held, and no other byte; the inputs are only read.
 * Non-finite values (here and in the statistics and the energy score): the comparisons are IEEE - a NaN sample counts in no
 * c_n, in neither rank nor ties - and NaN and +-Inf flow through the arithmetic of the formulas as written (an infinite
 * |d_n| against an infinite c_n d_n is NaN), in the one output element whose set holds them and in no other. */
SNSDE_API int snsde_sample_crps(const float* ys, const float* target, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                int32_t width, int32_t fair, float* crps, float* rank, float* ties, void* hip_stream);

/* Adjoint of snsde_sample_crps: with grad_crps (outer, groups, width) = g, and sign(0) = 0 (what |.| differentiates to),
 *     grad_ys[o, m, g, s, w] = g * (sign(d_n) / N - c_n / (N D))
 *     grad_target[o, g, w]   = -(g * sum_n sign(d_n)) / N                 (optional, NULL = not wanted)
 * which is autograd of the pairwise statement, ties included.  The counts are formed again from ys (no rank plane is saved);
 * every element of grad_ys is written; rank and ties carry no gradient.  The same ownership, errors and guarantees. */
SNSDE_API int snsde_sample_crps_backward(const float* grad_crps, const float* ys, const float* target, int64_t outer, int32_t members,
                                         int64_t groups, int32_t samples, int32_t width, int32_t fair, float* grad_ys, float* grad_target,
                                         void* hip_stream);

/* Quantiles of the pooled sample set by linear interpolation of order statistics (torch.quantile's 'linear' rule).  x_(k) is the
 * sample whose permutation rank r_n = #{j : x_j < x_n} + #{j < n : x_j == x_n} (ties broken by index) equals k.  For each of
 * the n_q requested levels the caller gives, from pos = q (N - 1) in double, k[i] = floor(pos) and frac[i] = (float)(pos - k[i]):
 *     out[i, o, g, w] = x_(k[i])                                                   where frac[i] == 0
 *                     = fmaf(frac[i], x_(k[i] + 1) - x_(k[i]), x_(k[i]))           otherwise
 * A sample set that holds a NaN has no order: out is NaN at every level (torch.quantile's rule; a NaN is given no rank, every wave
 * flags the NaNs of its quarter and the epilogue reads no order statistic of a flagged column - the same bits on every launch).
 * A set with +-Inf and no NaN follows the formula: an order statistic may be +-Inf, and interpolating (frac[i] != 0) from -Inf or
 * between equal infinities is NaN.
 * out is (n_q, outer, groups, width).  k and frac are HOST arrays of n_q entries, copied into the kernel's argument struct: no
 * device allocation, capturable.  SNSDE_ERR_DIMS also for n_q outside 1 .. 8, k[i] outside [0, N - 1], frac[i] outside [0, 1),
 * and k[i] == N - 1 with frac[i] != 0.  SNSDE_ERR_NULL: ys, k, frac or out NULL. */
SNSDE_API int snsde_sample_quantiles(const float* ys, int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                     int32_t n_q, const int32_t* k, const float* frac, float* out, void* hip_stream);

/* Adjoint of snsde_sample_quantiles: grad_out (n_q, outer, groups, width) = g_i; the ranks are formed again from ys,
 *     grad_ys[n] = sum_i ( g_i (1 - frac[i]) [r_n == k[i]] + g_i frac[i] [r_n == k[i] + 1, frac[i] != 0] ),   i ascending
 * and exact zeros everywhere else; every element of grad_ys is written.  In a set that holds a NaN (out is NaN there and has no
 * derivative) the result is still a function of the inputs alone: a NaN sample has no rank and gets an exact zero, the F finite
 * samples rank 0 .. F-1 among themselves and get the terms of the ranks they hold, and the terms of ranks >= F go nowhere. */
SNSDE_API int snsde_sample_quantiles_backward(const float* grad_out, const float* ys, int64_t outer, int32_t members, int64_t groups,
                                              int32_t samples, int32_t width, int32_t n_q, const int32_t* k, const float* frac,
                                              float* grad_ys, void* hip_stream);

/* ---- weighted sample sets: statistics, CRPS and quantiles of sample paths that carry log-weights ---------------------------
 * The six calls below are the weighted forms of snsde_sample_stats, snsde_sample_crps, snsde_sample_quantiles and their adjoints
 * (csrc/snsde_weighted.hip); the unweighted calls keep their kernels and their bits.  ys is viewed as above, and logw is
 * (outer, groups, N): one log-weight a_n per pooled path n = m S + s of an input row (N = M S; the statistics take members = 1,
 * N = S and outer folded into groups), shared by the `width` columns of the group - a particle filter's (T, B, S) log-weights
 * against its (T, B S, H) states.  N > 256 is SNSDE_ERR_DIMS in all six.
 * Normalisation, per group, by one wave before any sample is read (lane l holds a_n for n = l, 64 + l, 128 + l, 192 + l):
 *     mx  = fmaxf over all a_n (fmaxf skips a NaN)
 *     e_n = expf(a_n - mx), the difference rounded once
 *     P   = ((T_0 + T_1) + T_2) + T_3,  T_i = the sum of e_(64 i + l) over the 64 lanes l by the butterfly
 *           v_l <- v_l + v_(l xor s), s = 32, 16, 8, 4, 2, 1, with zeros in the places past N: a 256-leaf tree whose shape is a
 *           function of N alone (not of the grid, the width or the tile); nine additions deep
 *     w_n = e_n / P
 *     D'  = sum_n t_n over the same tree, t_n = w_n * (1 - w_n), each operation rounded once: the weighted (N - 1) / N, summed
 *           from non-negative terms (no cancellation near collapse)
 * Dead samples: a sample with e_n == 0 (a -Inf weight, or expf underflowed) in a group whose P is a number is dead.  It is
 * selected out, never multiplied: its value - NaN and +-Inf included - reaches no output and no gradient, its own gradient is an
 * exact zero, and the quantiles rank the live samples only.
 * Unusable weight sets: a group whose weights are all -Inf (mx = -Inf, e_n = expf(NaN)), or that holds a NaN or a +Inf weight,
 * has P = NaN and with it every w_n = NaN, 0 / NaN included: nothing is selected out and NaN reaches every output and gradient
 * element of the group by the arithmetic (the quantile calls, whose value is a selection, write NaN where P is NaN).  No other
 * group is affected.  A live sample that is NaN or +-Inf flows through the formulas as written.
 * The weights carry no gradient: the adjoints below are those with the weights fixed.
 * All six: enqueue-only, no workspace, no atomics, capturable; the same bits on every launch, whatever the grid and the alignment
 * of the pointers; every element of every output given is written and no other byte; the inputs are only read.  All pointers
 * device, fp32, contiguous.  Every check happens before the launch. */

/* Weighted mean and reliability-weights unbiased variance.  ys (groups, samples, width), logw (groups, samples); a wave owns one
 * (group, 64 adjacent columns) item, a lane one column, walked n ascending over the live samples, twice:
 *     mean = sum_n fmaf(w_n, x_n, .)
 *     var  = (sum_n fmaf(w_n, d_n * d_n, .)) / D',  d_n = x_n - mean         (optional, NULL = not wanted)
 * At equal weights D' = (S - 1) / S and var is the / (S - 1) estimator; with a single live sample var = 0 / 0 = NaN by the formula
 * (mean is that sample).  SNSDE_ERR_NULL: ys, logw or mean NULL.  SNSDE_ERR_DIMS: a non-positive extent, samples > 256, var with
 * samples < 2, an element count beyond 63 bits. */
SNSDE_API int snsde_sample_stats_weighted(const float* ys, const float* logw, int64_t groups, int32_t samples, int32_t width,
                                          float* mean, float* var, void* hip_stream);

/* Adjoint of snsde_sample_stats_weighted with the weights fixed: with c = (2 grad_var) / D',
 *     grad_ys[g, n, w] = w_n * fmaf(c, x_n - mean, grad_mean)       (grad_var NULL: w_n * grad_mean; ys and mean are then not read)
 * and an exact zero for a dead sample.  The weights are normalised again from logw.  The same ownership, errors and guarantees. */
SNSDE_API int snsde_sample_stats_weighted_backward(const float* grad_mean, const float* grad_var, const float* ys, const float* logw,
                                                   const float* mean, int64_t groups, int32_t samples, int32_t width, float* grad_ys,
                                                   void* hip_stream);

/* Weighted CRPS.  ys (outer, M, G, S, W), target (outer, G, W), logw (outer, G, N); tiles and quarters as snsde_sample_crps.  With
 * d_n = x_n - y and, over j ascending (IEEE comparisons; a dead j adds an exact zero),
 *     L_n = sum_j w_j [x_j < x_n],   U_n = sum_j w_j [x_j > x_n],   C_n = L_n - U_n
 *     crps = sum_n w_n |d_n| - (sum_n (w_n C_n) d_n) / D            D = D' (fair != 0) or 1
 *          = E_w |X - y| - sum_ij w_i w_j |x_i - x_j| / (2 D)
 *     rank = sum_n w_n [x_n < y],  ties = sum_n w_n [x_n == y]      the weighted PIT pieces, in [0, 1]; each optional, NULL = not wanted
 * over the live n.  Summation order: inside a quarter, n ascending, A = fmaf(w_n, |d_n|, A), B = fmaf(w_n * C_n, d_n, B), rank and
 * ties by fmaf(w_n, 0 or 1, .); the four quarter sums are added k ascending; then crps = A - B / D.  Fair with one live sample is
 * 0 / 0 = NaN by the formula.  SNSDE_ERR_NULL: ys, target, logw or crps NULL.  SNSDE_ERR_DIMS: a non-positive extent, N > 256, fair
 * with N < 2, an element count beyond 63 bits.  SNSDE_ERR_LDS: the device refuses the slab (N * 256 bytes) plus the weight rows. */
SNSDE_API int snsde_sample_crps_weighted(const float* ys, const float* target, const float* logw, int64_t outer, int32_t members,
                                         int64_t groups, int32_t samples, int32_t width, int32_t fair, float* crps, float* rank,
                                         float* ties, void* hip_stream);

/* Adjoint of snsde_sample_crps_weighted with the weights fixed, sign(0) = 0:
 *     grad_ys[n]  = g * (w_n * (sign(d_n) - C_n / D))                       an exact zero for a dead sample
 *     grad_target = -(g * sum_n fmaf(w_n, sign(d_n), .))                    quarters as above (optional, NULL = not wanted)
 * The C_n are formed again from ys and the weights; no plane is saved.  The same ownership, errors and guarantees. */
SNSDE_API int snsde_sample_crps_weighted_backward(const float* grad_crps, const float* ys, const float* target, const float* logw,
                                                  int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width,
                                                  int32_t fair, float* grad_ys, float* grad_target, void* hip_stream);

/* Weighted quantiles at the n_q levels q[i] in [0, 1] (a HOST array, copied into the kernel's argument struct); out is
 * (n_q, outer, groups, width).  Only the F live samples are ranked: r_n = #{live j : x_j < x_n} + #{live j < n : x_j == x_n},
 * A_n = the sum of w_j over the live j ranked before n, added j ascending, and the node of sample n is
 *     p_n = A_n / (1 - w_n);     by definition p = 0 for rank 0 and p = 1 for rank F - 1 (rank 0 first)
 * - the C = 1 member of the weighted-percentile family, r / (N - 1) at equal weights (torch.quantile's linear rule).  For a level q:
 * lo = the sample of largest rank with p <= q, hi = the sample of rank r_lo + 1 (picked by the integer ranks, whatever the rounding
 * of p), frac = clamp((q - p_lo) / (p_hi - p_lo), 0, 1) and
 *     out = x_lo                                     where r_lo == F - 1 or frac == 0
 *         = fmaf(frac, x_hi - x_lo, x_lo)            otherwise
 * A live NaN sample makes every level of its column NaN; +-Inf follows the formula.  SNSDE_ERR_NULL: ys, logw, q or out NULL.
 * SNSDE_ERR_DIMS: as above, n_q outside 1 .. 8, a level outside [0, 1].  SNSDE_ERR_LDS: the device refuses the slab, the nodes
 * (N * 256 bytes each), the rank table (N * 64 bytes) and the weight rows. */
SNSDE_API int snsde_sample_quantiles_weighted(const float* ys, const float* logw, int64_t outer, int32_t members, int64_t groups,
                                              int32_t samples, int32_t width, int32_t n_q, const float* q, float* out, void* hip_stream);

/* Adjoint of snsde_sample_quantiles_weighted with the weights fixed: grad_out (n_q, outer, groups, width) = g_i; the brackets are
 * formed again,
 *     grad_ys[lo_i] += g_i * (1 - frac_i),   grad_ys[hi_i] += g_i * frac_i (where the value interpolates),   i ascending
 * and exact zeros elsewhere, a dead sample included.  A column that holds a live NaN (out is NaN: no derivative) gets zeros; a
 * group with an unusable weight set NaN.  Every element of grad_ys is written. */
SNSDE_API int snsde_sample_quantiles_weighted_backward(const float* grad_out, const float* ys, const float* logw, int64_t outer,
                                                       int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t n_q,
                                                       const float* q, float* grad_ys, void* hip_stream);

/* Energy score: the multivariate generalisation of the CRPS, ES = E||X - y|| - E||X - X'|| / 2.  ys viewed as (outer, M, G, S, W)
 * exactly as for snsde_sample_crps (members axis: addressing only, member stride G S W; pooled set of group g: x_n, n = m S + s,
 * N = M S).  Two vector modes:
 *   path == 0: the vector is the last axis, x_n in R^W, V = W; one score per (o, g): energy is (outer, groups);
 *   path != 0: the outer axis joins the vector, component v = o W + w, V = outer W; one score per g: energy is (groups) - the
 *              score of the WHOLE path, all output times by all channels as one vector, addressed in place (no permuted copy).
 * target y is (outer, groups, width) in both modes.  With r_n = ||x_n - y||_2, r_nj = ||x_n - x_j||_2 and D = N - 1 (fair != 0:
 * the unbiased estimator; N < 2 is then SNSDE_ERR_DIMS) or D = N,
 *     energy = (sum_n r_n) / N - (sum_{n<j} r_nj) / (N D)                       (the CRPS at V = 1)
 * Every squared distance is formed from differences, sum_v (x_nv - x_jv)^2, never from a Gram matrix or norms: samples that
 * nearly coincide do not cancel.  One workgroup per score; the N + 1 rows (row N: the observation) are paired in 4 x 4
 * micro-tiles of row blocks, dealt to the lanes, which keep their squared distances in registers while the columns pass through
 * LDS in chunks of 16 (lanes past V stage zeros and store nothing); N > 256 is SNSDE_ERR_DIMS.  Summation order, a function of
 * (N, V, fair) only: a squared distance is one fmaf(d, d, .) chain over v ascending; after one sqrtf each, the 16 terms of a
 * tile (tile t = bj (bj + 1) / 2 + bi of row blocks bi <= bj, masked pairs as +0) are added as a balanced binary tree, the tiles
 * of a lane (t = lane + k THREADS) k ascending, the lanes of a wave by a butterfly (xor 1, 2, .., 32), the waves in order - the
 * pairs with the observation and the pairs among samples separately - then one division each and the subtraction.  THREADS = 64
 * for N <= 39, else 256.  No atomics, no dependence on the grid, the pointer alignment or `members`: the same bits on every
 * launch, and a pooled call gives the bits of the members = 1 call on the permuted (outer, G, M S, W) tensor.  Enqueue-only, no
 * workspace, capturable.  All pointers device, fp32, contiguous.  SNSDE_ERR_NULL: ys, target or energy NULL.  SNSDE_ERR_DIMS: a
 * non-positive extent, N > 256, fair with N < 2, an element count beyond 63 bits. */
SNSDE_API int snsde_sample_energy(const float* ys, const float* target, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                  int32_t width, int32_t fair, int32_t path, float* energy, void* hip_stream);

/* Adjoint of snsde_sample_energy: with grad_energy = g ((outer, groups), or (groups) under path), u(d) = d / ||d|| and u(0) = 0
 * (what the norm differentiates to in torch.linalg.vector_norm and torch.cdist: coincident samples and a sample on the
 * observation give finite gradients),
 *     grad_ys[n]  = g * ( u(x_n - y) / N - sum_{j != n} u(x_n - x_j) / (N D) )
 *     grad_target = -g * sum_n u(x_n - y) / N                                   (optional, NULL = not wanted)
 * The distances are formed again as in the forward; each pair leaves w = (1 / r, or 0 where r == 0) * (1 / N with the
 * observation, -1 / (N D) among samples) in an LDS plane of the lower triangle's 4 x 4 blocks (137 KB at N = 256: no workspace),
 * and a second pass over the columns writes g * sum_j w_nj (x_nv - x_jv), j ascending over the N + 1 rows, one fmaf each, for
 * every row n of every column (row N: grad_target).  Every element of grad_ys is written.  The same errors and guarantees;
 * SNSDE_ERR_NULL: grad_energy, ys, target or grad_ys NULL. */
SNSDE_API int snsde_sample_energy_backward(const float* grad_energy, const float* ys, const float* target, int64_t outer, int32_t members,
                                           int64_t groups, int32_t samples, int32_t width, int32_t fair, int32_t path, float* grad_ys,
                                           float* grad_target, void* hip_stream);

/* Energy score of a WEIGHTED and / or PARTIALLY OBSERVED sample set: the kernel of snsde_sample_energy
 * (csrc/snsde_energy.hip), of which weights and mask are compile-time variants; the unweighted, unmasked call keeps its bits.
 * Layout, pooling (n = m S + s, N = M S <= 256), `path` and `fair` as for snsde_sample_energy.  A call with neither weights nor
 * mask runs the variant snsde_sample_energy runs, and gives its bits.
 * Mask.  mask (NULL = none) has the shape of target, (outer, groups, width); a coordinate is observed where mask != 0 - the value
 * is a flag, a fractional value does NOT weigh.  With mask NULL and nan_missing != 0 a coordinate is observed where target is not
 * NaN.  Both are decided inside the kernel by the thread that stages the column: no extra launch, no mask tensor made from isnan.
 * With O the observed coordinates of a score (under path: of all outer * width components) every distance is taken over O only,
 *     r_n = ||(x_n - y)|_O||,   r_nj = ||(x_n - x_j)|_O||
 * and an unobserved coordinate is selected out, never multiplied: nothing of ys or target is read there (zeros are staged for
 * every row of the column, and fmaf(0, 0, acc) leaves each chain untouched), so NaN / Inf there reaches no value and no gradient,
 * and grad_ys and grad_target there are exact zeros written by selection - also where grad_energy is NaN or Inf.  A score whose O
 * is empty is 0 (NaN with an unusable weight set) with zero gradients.  A masked score has the bits of the unmasked kernel on the
 * vectors compacted to their observed columns; a mask of all ones without weights gives the bits of snsde_sample_energy.
 * Weights.  logw (NULL = none) is (outer, groups, N), or (groups, N) under path: one log-weight per pooled path of a score.  They
 * are normalised exactly as for the weighted calls above - mx, e_n = expf(a_n - mx), P, w_n = e_n / P, D' = sum w_n (1 - w_n) over
 * the same 256-leaf tree - by wave 0, once per score, while the loads of the first chunk of columns are in flight.  With D = D'
 * (fair != 0) or 1,
 *     energy = sum_n w_n r_n - (sum_{n<j} w_n w_j r_nj) / D
 * which at w = 1 / N is the formula of snsde_sample_energy for both values of fair, and at integer multiplicities with fair == 0
 * the unweighted score of the replicated set.  A dead sample (e_n == 0 where P is a number) is selected out of every pair; in a
 * group whose P is NaN every w_n is NaN and so is every value of the group (its gradients at unobserved coordinates stay exact
 * zeros), and no other group is touched.  One live sample under fair gives D' = 0 and 0 / 0 = NaN, as the weighted variance does.
 * Summation order, a function of (N, V, fair) only: the squared distances, sqrtf and the tile / lane / butterfly / wave order of
 * snsde_sample_energy; the term of a pair is fl(fl(w_i w_j) r_ij) with w = 1 for the observation, dead and masked pairs entering
 * as +0; then energy = A - B / D' (fair) or A - B.  Without logw: A / N - B / (N D), the arithmetic of snsde_sample_energy.
 * No atomics, no workspace, no dependence on the grid or the pointer alignment; enqueue-only, capturable; every element of energy
 * is written and no other byte.  All pointers device, fp32, contiguous.  SNSDE_ERR_NULL: ys, target or energy NULL.
 * SNSDE_ERR_DIMS: a non-positive extent, N > 256, fair with N < 2, an element count beyond 63 bits.  SNSDE_ERR_LDS: the device
 * refuses the chunk, the weight rows and - backward - the plane (156 160 bytes at N = 256).  Every check precedes the launch. */
SNSDE_API int snsde_sample_energy_weighted(const float* ys, const float* target, const float* logw, const float* mask, int64_t outer,
                                           int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t fair, int32_t path,
                                           int32_t nan_missing, float* energy, void* hip_stream);

/* Adjoint of snsde_sample_energy_weighted with the weights fixed: with grad_energy = g, u(d) = d / ||d|| over the observed
 * coordinates and u(0) = 0,
 *     grad_ys[n]  = g * ( w_n u(x_n - y) - sum_{j != n} w_n w_j u(x_n - x_j) / D )        live n, observed coordinates
 *     grad_target = -g * sum_n w_n u(x_n - y)                                             (optional, NULL = not wanted)
 * (without logw: 1 / N and 1 / (N D), the adjoint of snsde_sample_energy).  The distances are formed again; the plane entry of a
 * pair is (1 / r, or 0 where r == 0) * c, c = fl(w_i w_j) with the observation and fl(fl(w_i w_j) * (-1 / D)) among samples, 0 where
 * a row is dead; the second pass stages the rows of a dead sample as zeros and gives row n of a column g * sum_j c_nj (x_nv - x_jv),
 * j ascending over the N + 1 rows, one fmaf each.  The writer selects an exact zero for every row of an unobserved column and for
 * the whole row of a dead sample, whatever ys, target and g hold there.  One live sample under fair: NaN, the formula's 0 / 0.
 * Every element of grad_ys (and of grad_target) is written and no other byte.  The same errors and guarantees; SNSDE_ERR_NULL:
 * grad_energy, ys, target or grad_ys NULL. */
SNSDE_API int snsde_sample_energy_weighted_backward(const float* grad_energy, const float* ys, const float* target, const float* logw,
                                                    const float* mask, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                                    int32_t width, int32_t fair, int32_t path, int32_t nan_missing, float* grad_ys,
                                                    float* grad_target, void* hip_stream);

/* Masked Gaussian log-likelihood of sample paths and its importance-weighted (IWAE) bound: the training objective for data with
 * missing entries.  ys viewed as (outer, M, G, S, W) exactly as for snsde_sample_energy with path != 0: pooled sample
 * n = m S + s, N = M S; vector component v = o W + w, V = outer W; addressed in place (no permuted copy).  target y and mask m
 * are (outer, groups, width); an element is observed where m_v != 0.  The observation noise is one scalar std > 0: the caller
 * computes logvar = 2 log(std) and inv_var = exp(-logvar) in double and passes both as float.
 *     logpx[g, n] = sum_{v observed} m_v (-1/2) (log 2 pi + logvar + (y_v - x_nv)^2 inv_var)                 (groups, N)
 *     count[g]    = sum_{v observed} m_v                                                                     (groups)
 *     norm != 0:    logpx[g, .] is divided by count[g] where count[g] > 0 and stays 0 where count[g] == 0 (a deliberate
 *                   difference from dividing 0 by 0)
 *     bound[g]    = logsumexp_n(logpx[g, n] + logw[g, n]) - log N                                            (groups)
 *     sqerr[g]    = sum_{v observed} m_v (y_v - xbar_v)^2,  xbar_v = (sum_n x_nv) / N                        (groups)
 * logw (groups, N) is an optional log importance weight (-kl_coef * kl, the per-path KL column of a latent solve); NULL = 0.
 * sqerr is the numerator of the masked mean squared error of the sample mean (the caller divides by count): a metric.
 * Select, never multiply: an element with m_v == 0 enters no sum (exact +0; its samples are not loaded) and receives an exact-zero
 * gradient, whatever target or ys hold there (NaN-marked missing data is accepted as it is).  Fractional mask values weigh.
 * A NaN in an observed element of path n makes logpx[g, n], bound[g] and sqerr[g] NaN and touches no other group; the
 * logsumexp subtracts the maximum (all -Inf gives -Inf, a NaN gives NaN).
 * One workgroup of 256 threads per group (grid stride beyond 8192 groups).  L = min(32, largest power of two <= 256 / N) lanes
 * share a sample; the group's N x V slab passes once from memory, coalesced along w, through LDS in chunks of CW = 64 L columns
 * as the residuals d_nv = y_v - x_nv (row stride CW + L mod 32 words: the transposed read of the per-sample sums is free of
 * bank conflicts); the thread that stages a column adds its residuals as they arrive.  Summation order, a function of (N, V) only:
 *   q_n = sum_v m_v d_nv^2: sub-lane l a chain q = fmaf(m_v d, d, q) over v = l (mod L) ascending, the L chains by a butterfly
 *   (xor 1, .., L / 2); count likewise with additions; logpx = -0.5f fmaf(inv_var, q, ((float)log 2 pi + logvar) count), then
 *   the division under norm;
 *   s_v = sum_n d_nv: n ascending inside each of RS = max(1, 4 / L) contiguous parts [k N / RS, (k + 1) N / RS), the parts in
 *   order; e_v = s_v / N; thread t a chain fmaf(m_v e_v, e_v, .) over v = t (mod min(CW, 256)) ascending; the 64 lanes of a
 *   wave by a butterfly (xor 1, .., 32), the four waves in order;
 *   bound: max_n a_n, a_n = logpx_n + logw_n; lane i a chain of expf(a_n - max) over n = i (mod 64) ascending, the lanes by a
 *   butterfly; max + logf(sum) - logf((float)N).
 * No atomics, no workspace, no dependence on the grid, the pointer alignment or `members`: the same bits on every launch, and a
 * pooled call gives the bits of the members = 1 call on the permuted tensor.  Every element of logpx, count, bound and sqerr is
 * written (a fully masked group included) and no other byte; the inputs are only read.  Enqueue-only, capturable.  All pointers device,
 * fp32, contiguous.  SNSDE_ERR_NULL: ys, target, mask, logpx, count, bound or sqerr NULL.  SNSDE_ERR_DIMS: a non-positive
 * extent, N > 256, logvar or inv_var not finite or inv_var <= 0 (a non-finite or non-positive std), an element count beyond 63 bits. */
SNSDE_API int snsde_sample_loglik(const float* ys, const float* target, const float* mask, const float* logw, int64_t outer,
                                  int32_t members, int64_t groups, int32_t samples, int32_t width, float logvar, float inv_var,
                                  int32_t norm, float* logpx, float* count, float* bound, float* sqerr, void* hip_stream);

/* Adjoint of snsde_sample_loglik: grad_logpx (groups, N) and grad_bound (groups), either may be NULL (none).  With logpx and
 * count as the forward left them, p_n = softmax_n(logpx[g, n] + logw[g, n]) (formed again in the kernel's prologue: <= 256
 * terms per group) and c[g, n] = (grad_logpx[g, n] + grad_bound[g] p_n) / (count[g] under norm, else 1; 0 where count == 0),
 *     grad_ys[n, v]   = c_n m_v (y_v - x_nv) inv_var                     (as ys; every element is written)
 *     grad_target[v]  = -sum_n grad_ys[n, v], n ascending in the lane that owns the column   (optional, NULL = not wanted)
 *     grad_logw[g, n] = grad_bound[g] p_n                                                    (optional, NULL = not wanted)
 * computed as ((c_n inv_var) m_v) (y_v - x_nv).  Unobserved elements of grad_ys and grad_target are exact +0.  sqerr, mask and
 * the variance carry no gradient.  Every element of grad_target and grad_logw, where given, is written too, and no other byte.
 * Elementwise over the slab: a workgroup per (group, 256 adjacent columns).  The same errors
 * and guarantees; SNSDE_ERR_NULL: ys, target, mask, logpx, count or grad_ys NULL. */
SNSDE_API int snsde_sample_loglik_backward(const float* grad_logpx, const float* grad_bound, const float* ys, const float* target,
                                           const float* mask, const float* logw, const float* logpx, const float* count, int64_t outer,
                                           int32_t members, int64_t groups, int32_t samples, int32_t width, float logvar, float inv_var,
                                           int32_t norm, float* grad_ys, float* grad_target, float* grad_logw, void* hip_stream);

/* snsde_sample_loglik under a log standard deviation per channel or per entry in place of the one scalar variance.  ys, target,
 * mask, logw, the outputs and the pooled layout exactly as there.  log_std holds ls = log(std):
 *     noise_mode = SNSDE_NOISE_CHANNEL: (width); column v = o width + w of the path vector reads entry w
 *     noise_mode = SNSDE_NOISE_ENTRY:   (outer, groups, width), the shape of target and mask
 *     logpx[g, n] = sum_{v observed} m_v (-1/2) (log 2 pi + 2 ls_v + (y_v - x_nv)^2 exp(-2 ls_v))           (groups, N)
 * count, norm, bound and sqerr as for snsde_sample_loglik (sqerr is not weighed by the noise); count has that call's bits.
 * Select, never multiply, covers the noise: ls_v is loaded only where m_v != 0, so NaN or Inf at an unobserved entry reaches
 * nothing; a NaN ls_v at an observed entry makes every logpx[g, .], bound[g] of its group NaN (in channel mode: of every group
 * that observes the channel) and touches no other group.  The values of log_std are not checked.
 * The decomposition of snsde_sample_loglik; the thread that stages a column forms iv_v = expf(-2 ls_v), u_v = m_v iv_v and
 * t_v = m_v fmaf(2, ls_v, (float)log 2 pi) once per column (+0 where unobserved) into LDS beside m_v.  Summation order, a
 * function of (N, V) only:
 *   q_n = sum_v u_v d_nv^2: sub-lane l a chain q = fmaf(u_v d, d, q) over v = l (mod L) ascending, the L chains by a butterfly
 *   (xor 1, .., L / 2); count = sum m_v and lv = sum t_v by the same chains and butterfly, additions;
 *   logpx = -0.5f (q_n + lv), then the division under norm; sqerr and bound as for snsde_sample_loglik.
 * The two modes run the same arithmetic: channel mode gives the bits of entry mode on the broadcast plane.  No atomics, no
 * workspace, the same bits on every launch and for every pointer alignment; a pooled call gives the bits of the members = 1 call on
 * the permuted tensor.  Every element of logpx, count, bound and sqerr is written and no other byte; the inputs are only read.
 * Enqueue-only, capturable.  All pointers device, fp32, contiguous.  SNSDE_ERR_NULL: ys, target, mask, log_std, logpx, count,
 * bound or sqerr NULL.  SNSDE_ERR_DIMS: a non-positive extent, N > 256, a noise_mode other than the two, an element count
 * beyond 63 bits. */
#define SNSDE_NOISE_CHANNEL 0
#define SNSDE_NOISE_ENTRY 1
SNSDE_API int snsde_sample_loglik_noise(const float* ys, const float* target, const float* mask, const float* logw,
                                        const float* log_std, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                        int32_t width, int32_t noise_mode, int32_t norm, float* logpx, float* count, float* bound,
                                        float* sqerr, void* hip_stream);

/* Adjoint of snsde_sample_loglik_noise, the log-std included.  grad_logpx, grad_bound, p_n and c[g, n] as for
 * snsde_sample_loglik_backward; with d = y_v - x_nv, iv_v = expf(-2 ls_v), u_v = m_v iv_v:
 *     grad_ys[n, v]     = (c_n u_v) d                                      (as ys; every element is written)
 *     grad_target[v]    = -sum_n grad_ys[n, v], n ascending               (optional, NULL = not wanted)
 *     grad_logw[g, n]   = grad_bound[g] p_n                               (optional, NULL = not wanted)
 *     grad_log_std[v]   = m_v r_v, r_v the chain r = fmaf(c_n, fmaf(d iv_v, d, -1), r) over n ascending
 *                         (optional, NULL = not wanted; ALWAYS the per-entry plane (outer, groups, width), in both modes)
 * The lane that owns a column forms all of them in one walk.  Unobserved elements of grad_ys, grad_target and grad_log_std are
 * exact +0 and their ls_v is not loaded.  In channel mode the gradient of the (width) vector is the column sum of grad_log_std:
 * snsde_sample_loglik_noise_reduce.  Every element of each output given is written and no other byte; no atomics; the same
 * bits on every launch.  A workgroup per (group, 256 adjacent columns).  The errors of the forward; SNSDE_ERR_NULL: ys, target,
 * mask, log_std, logpx, count or grad_ys NULL. */
SNSDE_API int snsde_sample_loglik_noise_backward(const float* grad_logpx, const float* grad_bound, const float* ys, const float* target,
                                                 const float* mask, const float* logw, const float* log_std, const float* logpx,
                                                 const float* count, int64_t outer, int32_t members, int64_t groups, int32_t samples,
                                                 int32_t width, int32_t noise_mode, int32_t norm, float* grad_ys, float* grad_target,
                                                 float* grad_logw, float* grad_log_std, void* hip_stream);

/* grad_channel[w] = sum_r grad_entry[r, w]: the (rows, width) plane grad_log_std of snsde_sample_loglik_noise_backward
 * (rows = outer groups) summed to the (width) gradient of a per-channel log_std, in a fixed order that depends on rows and
 * width alone.  With R = SNSDE_LOGLIK_NOISE_REDUCE_ROWS and P = ceil(rows / R): stage 1, partial[k, w] = the rows
 * [k R, min(rows, (k + 1) R)) of column w added ascending, k < P; stage 2, grad_channel[w] = partial[0, w] + partial[1, w] + ..
 * ascending.  partial is the caller's (P, width) floats - the library allocates nothing; where P == 1 stage 1 writes
 * grad_channel itself and partial may be NULL.  Every element of grad_channel (and of partial, where P > 1) is written and no
 * other byte; grad_entry is only read.  No atomics: deterministic, independent of alignment, enqueue-only, capturable (one or
 * two launches).  SNSDE_ERR_NULL: grad_entry or grad_channel NULL, partial NULL where P > 1.  SNSDE_ERR_DIMS: rows or width
 * not positive, rows width beyond 63 bits. */
#define SNSDE_LOGLIK_NOISE_REDUCE_ROWS 64
SNSDE_API int snsde_sample_loglik_noise_reduce(const float* grad_entry, int64_t rows, int32_t width, float* partial,
                                               float* grad_channel, void* hip_stream);

/* Classification with sample paths: the predictive (model-average) negative log-likelihood of a label, the expected
 * cross-entropy, the predictive distribution and the split of its entropy.  logits viewed as (outer, M, G, S, C) exactly as ys
 * for snsde_sample_crps: pooled path n = m S + s, N = M S <= 256; one result per (o, g).  labels are int32 (outer, groups) or
 * NULL; logw (outer, groups, N) is an optional log importance weight as for snsde_sample_loglik (NULL = 0); class_weight (C
 * classes; two for binary) is optional (NULL = 1).  binary != 0: the stored width is 1 and the two class logits of a path
 * are (0, z) (a logit for BCE-with-logits; class_weight = (1, pos_weight) gives BCEWithLogitsLoss(pos_weight)).
 * With lp_n[c] = z_n[c] - logsumexp_c z_n, a_n = lp_n[y], w = class_weight[y]:
 *     logp[g, n]  = a_n                                                                              (outer, groups, N)
 *     nll[g]      = -w (logsumexp_n(a_n + logw_n) - log N)          the predictive negative log-likelihood
 *     xent[g]     = -w (1 / N) sum_n a_n                            the expected cross-entropy (>= nll where logw = 0)
 *     probs[g, c] = (1 / N) sum_n exp(lp_n[c])                      (outer, groups, C); binary: (outer, groups, 1), class 1
 *     entropy[g]  = -sum_c pbar_c log pbar_c   (0 log 0 = 0)        total uncertainty
 *     expent[g]   = -(1 / N) sum_n sum_c p_nc lp_nc   (p = 0: 0)    expected entropy; entropy - expent is the mutual information
 * Every logsumexp subtracts its maximum, and lp is formed as (z - max) - log sum exp(z - max): logits of magnitude 1e4 neither
 * overflow nor lose the answer.  A -Inf logit is a class of probability zero (exact zeros).  label < 0 (or labels == NULL): the
 * row is unlabelled, logp, nll and xent are exact +0 and probs, entropy, expent are computed all the same.  label >= the number
 * of classes: NaN in logp, nll and xent.  The label only selects among values already read, by comparison with the column index:
 * it forms no address.  A NaN logit in path n makes logp[g, n] and the group's nll, xent, probs, entropy and expent NaN and
 * touches no other group.
 * A workgroup of 256 threads per pack of GP adjacent groups (grid stride beyond 4096 packs).  L = min(64, least power of two
 * >= C) lanes share a row, R = 256 / L rows at a time; GP = 1 for C > 64, else the largest power of two <= max(1, R / N).
 * The pack's slab goes once from memory into LDS, coalesced along c, where GP N C <= 24576 floats, and everything else reads
 * LDS; a larger one is read from memory by the row sums and a second time (from L2) for probs.  Summation order, a function of (N, C) only:
 *   row: lane l the online pair (m, s) over c = l (mod L) ascending - z > m: s = s expf(m - z) + 1, m = z; else s += expf(z - m)
 *   (shift 0 while m = -Inf) - then the row's maximum m' by a butterfly over the L lanes, each lane's s scaled once,
 *   s expf(m - m'), and the L products added by a butterfly (xor 1, .., L / 2); ls = logf(s); lp_c = (z_c - m') - ls.
 *   binary: m = max(0, z), s = expf(0 - m) + expf(z - m).
 *   probs: C <= 64: thread (group, part k, column c) adds p_nc = expf(lp_nc) over n ascending in its part
 *   [k N / RS, (k + 1) N / RS), RS = min(16, R / GP), then the parts k ascending; C > 64: thread t the columns c = t (mod 256),
 *   n ascending; then / N.  The same thread adds p lp as it goes (C > 64: columns outer, rows inner), then the parts in order;
 *   entropy adds -pbar logf(pbar) (C > 64: c ascending per thread); both then over the min(C', 64) column lanes (C' = L, or 256
 *   for C > 64) by a butterfly (xor 1, ..) and for C > 64 over the four waves in order.  binary: pbar_0 is summed like pbar_1.
 *   nll, xent: a'_n = a_n + logw_n; TN = min(64, 256 / GP) lanes per group; max over n; lane i the chains sum += expf(a'_n - max)
 *   and sum += a_n over n = i (mod TN) ascending, the lanes by a butterfly; nll = -w (max + logf(sum) - logf((float)N)), xent =
 *   -w (sum / N).  A NaN a'_n gives NaN, an infinite maximum max - logf(N).
 * No atomics, no workspace, no dependence on the grid, the pointer alignment or `members`: the same bits on every launch, and a
 * pooled call gives the bits of the members = 1 call on the permuted tensor.  Every element of the six outputs is written (an
 * unlabelled group included) and no other byte; the inputs are only read.  Enqueue-only, capturable.  All pointers device,
 * contiguous; fp32 but labels.  SNSDE_ERR_NULL: logits or an output NULL.  SNSDE_ERR_DIMS: a non-positive extent, N > 256,
 * binary with width != 1, an element count beyond 63 bits. */
SNSDE_API int snsde_sample_class(const float* logits, const int32_t* labels, const float* logw, const float* class_weight,
                                 int64_t outer, int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t binary,
                                 float* logp, float* nll, float* xent, float* probs, float* entropy, float* expent, void* hip_stream);

/* Adjoint of snsde_sample_class: grad_nll (outer, groups), grad_xent (outer, groups) and grad_logp (outer, groups, N), each may
 * be NULL (none).  The row statistics are formed again as in the forward; with r_n = softmax_n(a_n + logw_n) (expf(a'_n - max) /
 * sum, the forward's max and sum; the slab staged as in the forward) and k_n = w (grad_nll r_n + grad_xent / N) - grad_logp_n,
 *     grad_logits[n, c] = k_n (p_nc - [c == y])                  (as logits; every element is written)
 *     grad_logw[g, n]   = -w grad_nll[g] r_n                      (optional, NULL = not wanted)
 * binary: the gradient of z is the class-1 column.  An unlabelled group's slab and grad_logw row are exact +0; a label >= the
 * number of classes gives NaN in that group's rows.  Every element of grad_logw, where given, is written too, and no other byte.
 * probs, entropy, expent and class_weight carry no gradient.  The same
 * errors and guarantees; SNSDE_ERR_NULL: logits or grad_logits NULL. */
SNSDE_API int snsde_sample_class_backward(const float* grad_nll, const float* grad_xent, const float* grad_logp, const float* logits,
                                          const int32_t* labels, const float* logw, const float* class_weight, int64_t outer,
                                          int32_t members, int64_t groups, int32_t samples, int32_t width, int32_t binary,
                                          float* grad_logits, float* grad_logw, void* hip_stream);

/* ---- particle filtering on sample paths -------------------------------------------------------
 * One step of the bootstrap particle filter: weigh the S paths of every group by the newest observation and resample them.
 * state viewed as (groups, samples, width) = (G, S, W): the (B S, H) last state of a sampled solve, path b S + s; an ensemble
 * result folds its members into the groups (members are never pooled: a particle does not change model).  logw (G, S) is the
 * carried log-weight, loginc (G, S) the optional log-likelihood increment (NULL = 0), u the uniforms in [0, 1) the caller drew:
 * (G) for systematic resampling, (G, S) where stratified != 0.  Per group, n and j in 0 .. S-1:
 *     a_n  = logw_n + loginc_n                  mx = max_n a_n                  e_n = expf(a_n - mx)
 *     P_n  = e_0 + .. + e_n
 *     logz = mx + logf(P_{S-1}) - logf((float)S)                                 logsumexp(a) - log S            (G)
 *     ess  = P_{S-1}^2 / sum_n e_n^2                                             the effective sample size      (G)
 * The group is resampled where threshold >= 1, or where ess < threshold S; threshold <= 0 never resamples.  Where resampled:
 *     t_j = ((j + u_j) / S) P_{S-1},  u_j = u[g] (stratified: u[g, j])
 *     ancestor[j]     = #{n < S-1 : P_n <= t_j}                                                                  (G, S) int32
 *     state_out[j, :] = state[ancestor[j], :]                                                                    (G, S, W)
 *     logw_out[j]     = logz                                                                                     (G, S)
 * and where not: ancestor[j] = j, state_out a copy of state, logw_out = a.  resampled[g] is 1 or 0 (int32).  Either way
 * logsumexp(logw_out) - log S = logz: the evidence is carried in the weights, and logw_out handed to snsde_sample_loglik as
 * logw makes its bound the running log marginal likelihood.
 * Special values.  A particle with e_n == 0 (a -Inf weight, or one so far below the maximum that expf gives 0) is never an
 * ancestor: P_n == P_{n-1} exactly, so nothing counts into it, and a t_j that rounds up to P_{S-1} behind dead trailing
 * particles (u the largest float below 1) is clamped to the last particle with e_n > 0 instead of S - 1.  (A u outside [0, 1)
 * or NaN is clamped into the first .. last such particle likewise.)  A group whose a are all -Inf is not resampled: ancestor
 * is the identity, state_out a copy, logw_out = a, ess = 0, logz = -Inf, resampled = 0.  A group that holds a NaN or a +Inf
 * in a is not resampled either: identity, copies, logw_out = a, ess = logz = NaN, resampled = 0; no other group is touched.
 * state is only moved, in 32-bit or 128-bit words: NaN, Inf and every other bit pattern arrive bit for bit.  S = 1 is legal:
 * the identity, ess = 1.
 * A workgroup of 256 threads per pack of GP adjacent groups (grid stride beyond 2048 packs), GP the largest power of two
 * <= max(1, min(256 / S, 4096 / (S W))); thread gp S + n is particle n of the pack's group gp.  Rows are gathered with 16-byte
 * accesses where W % 4 == 0 and state and state_out are 16-byte aligned, one float at a time otherwise: the same bits.
 * Summation order, a function of S only:
 *   a_n one rounded addition; mx by fmaxf over n ascending; e_n = expf(a_n - mx), the difference rounded once;
 *   P_n = P_{n-1} + e_n and q = fmaf(e_n, e_n, q): two sequential chains over n ascending in one thread (so P is non-decreasing
 *   whatever the rounding); ess = (P_{S-1} P_{S-1}) / q; logz = (mx + logf(P_{S-1})) - logf((float)S);
 *   t_j = (((float)j + u_j) / (float)S) P_{S-1}, every operation rounded once; the count by a binary search over P_0 .. P_{S-2}.
 * No atomics, no workspace, no dependence on the grid or the pointer alignment: the same bits on every launch.  Every element
 * of the six outputs is written and no other byte; the inputs are only read.  Enqueue-only, capturable.  All pointers device,
 * contiguous; fp32 but ancestor and resampled (int32).  Errors are returned before any launch.  SNSDE_ERR_NULL: state, logw,
 * u or an output NULL.  SNSDE_ERR_DIMS: a non-positive extent, S > 256, a NaN threshold, an element count beyond 63 bits,
 * state_out overlapping state. */
SNSDE_API int snsde_sample_resample(const float* state, const float* logw, const float* loginc, const float* u,
                                    int64_t groups, int32_t samples, int32_t width, int32_t stratified, float threshold,
                                    float* state_out, float* logw_out, int32_t* ancestor, float* ess, float* logz,
                                    int32_t* resampled, void* hip_stream);

/* The adjoint of snsde_sample_resample with the ancestors held fixed: ancestor, resampled (the forward's outputs, inputs here)
 * and with them u and the threshold are constants of the backward.  This is the estimator of the filtering variational
 * objectives (FIVO): the score-function term of the resampling decision is dropped.  Inputs: the gradients of the three
 * differentiable outputs, grad_state_out (G, S, W), grad_logw_out (G, S) and grad_logz (G), each of which may be NULL (= zero),
 * and the forward's logw, loginc (NULL = 0), ancestor (G, S) and resampled (G).  ess carries no gradient.  Outputs: grad_state
 * (G, S, W) and grad_a (G, S), the gradient of a = logw + loginc and so of logw and of loginc alike.  Per group, with
 * w_n = e_n / P_{S-1} (the softmax of a) formed again from logw and loginc:
 *     resampled:   grad_state[n, :] = sum_{j : ancestor[j] == n} grad_state_out[j, :]
 *                  grad_a[n]        = (grad_logz + sum_j grad_logw_out[j]) w_n            (every logw_out[j] is logz)
 *     kept:        grad_state[n, :] = grad_state_out[n, :]
 *                  grad_a[n]        = grad_logw_out[n] + grad_logz w_n
 * A group counts as resampled where resampled[g] != 0 and its a are summed (next paragraph); its ancestors need not be
 * monotone, and an ancestor outside [0, S) is the child of no particle: its row of grad_state_out is not read and no address
 * is formed from it.
 * Special values.  A particle with e_n == 0 receives an exact 0 from grad_logz and the weights' sum (whatever their value),
 * and, never an ancestor, an exact +0 row of grad_state where the group is resampled.  A group whose a are all -Inf, or that
 * holds a NaN or a +Inf, is the identity whatever resampled[g] says: grad_state = grad_state_out and grad_a = grad_logw_out bit
 * for bit, the grad_logz term an exact zero; no other group is touched.  grad_state_out is only moved and added: a row with
 * one child, and every kept row, arrives bit for bit, and a NaN reaches only the row of its ancestor.
 * The forward's geometry: a workgroup of 256 threads per pack of GP adjacent groups, thread gp S + n particle n of group gp;
 * 16-byte accesses where W % 4 == 0 and grad_state_out and grad_state are 16-byte aligned, one float at a time otherwise: the
 * same bits.  Order of the operations, a function of S and of ancestor only:
 *   a_n, mx, e_n and the chain P_n = P_{n-1} + e_n as the forward forms them; s = s + grad_logw_out[n] from 0, n ascending in one
 *   thread; c = grad_logz + s (kept: grad_logz); w_n = e_n / P_{S-1}; z_n = c w_n (e_n == 0: 0); grad_a[n] = z_n (kept:
 *   grad_logw_out[n] + z_n), every operation rounded once, no fused multiply-add;
 *   grad_state[n, :]: the row of the least child j moved, then the rows of the further children added in ascending j, one
 *   rounded addition each (the child lists are built per group in LDS: count, prefix, stable fill); no child: +0.
 * No atomics, no workspace, no dependence on the grid or the pointer alignment: the same bits on every launch.  Every element
 * of the two outputs is written and no other byte; the inputs are only read, each row of grad_state_out once at most.
 * Enqueue-only, capturable.  All pointers device, contiguous; fp32 but ancestor and resampled (int32).  Errors are returned
 * before any launch.  SNSDE_ERR_NULL: logw, ancestor, resampled or an output NULL.  SNSDE_ERR_DIMS: a non-positive extent,
 * S > 256, an element count beyond 63 bits, an output overlapping an input or the other output. */
SNSDE_API int snsde_sample_resample_backward(const float* grad_state_out, const float* grad_logw_out, const float* grad_logz,
                                             const float* logw, const float* loginc, const int32_t* ancestor,
                                             const int32_t* resampled, int64_t groups, int32_t samples, int32_t width,
                                             float* grad_state, float* grad_a, void* hip_stream);

SNSDE_API int         snsde_version(void);
/* SNSDE_OK when `version` == SNSDE_VERSION and the four sizes equal the library's sizeof(snsde_model / snsde_solve /
 * snsde_backward / snsde_head); SNSDE_ERR_ABI otherwise.  A size of 0 means "this binding does not declare that struct"
 * (a forward-only binding has no snsde_backward / snsde_head) and is not compared.  A binding calls it once after loading
 * the library.                                                                                                          */
SNSDE_API int         snsde_abi_check(int version, size_t sizeof_model, size_t sizeof_solve, size_t sizeof_backward, size_t sizeof_head);
SNSDE_API const char* snsde_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* SNSDE_H */
