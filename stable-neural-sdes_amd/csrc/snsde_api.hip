// C-ABI entry points of libsnsde.so (include/snsde.h): parameter layout, torchsde-style fixed-step
// time grid (host), argument validation and kernel dispatch.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "snsde_mfma_kernels.h"      // (MfmaPlan: host side only, no kernel is instantiated here)

namespace {

struct ParamEntry {
    char name[40];
    int64_t offset;
    int32_t rows, cols;  // bias / vectors: rows = n, cols = 0 ; theta: (1,1)
};

constexpr int MAX_PARAMS = 2 * (SNSDE_MAX_HIDDEN + 8) + 4;

int validate_model(const snsde_model* m) {
    if (!m) return SNSDE_ERR_NULL;
    if (m->input_channels <= 0 || m->hidden_channels <= 0 || m->hidden_hidden_channels <= 0 ||
        m->num_hidden_layers <= 0)
        return SNSDE_ERR_DIMS;
    if (m->num_hidden_layers - 1 > SNSDE_MAX_HIDDEN) return SNSDE_ERR_UNSUPPORTED;
    if (m->input_option < 0 || m->input_option > 6 || m->noise_option < 0 || m->noise_option > 19)
        return SNSDE_ERR_OPTION;
    if (m->activation < 0 || m->activation > SNSDE_ACT_SILU || m->drift_output < 0 || m->drift_output > SNSDE_DRIFT_TIMES_Y ||
        m->diffusion_output < 0 || m->diffusion_output > SNSDE_DIFFUSION_RAW_NET || m->time_feature < 0 ||
        m->time_feature > SNSDE_TIME_RAW)
        return SNSDE_ERR_OPTION;
    if (m->diffusion_output == SNSDE_DIFFUSION_RAW_NET && m->noise_option != 18 && m->noise_option != 19) return SNSDE_ERR_OPTION;
    const int io = m->input_option;
    // emb = Linear(2H, H) consumes cat[yy (HH), Xt (H)] and io 0 feeds Xt (H) to the HH-wide MLP:
    // both need HH == H (neuralsde.py:150-158, 206-210)
    if ((io == 0 || io == 2 || io == 4 || io == 6) && m->hidden_hidden_channels != m->hidden_channels)
        return SNSDE_ERR_DIMS;
    return SNSDE_OK;
}

// state_dict order of the reference Diffusion_model (neuralsde.py:142-179): direct parameters
// (theta, sigma, sigma_diag) first, then the sub-modules in definition order.
int build_params(const snsde_model* m, ParamEntry* e, int* count, int64_t* total) {
    int rc = validate_model(m);
    if (rc) return rc;
    const int C = m->input_channels, H = m->hidden_channels, HH = m->hidden_hidden_channels;
    const int io = m->input_option, no = m->noise_option;
    int n = 0;
    int64_t off = 0;
    auto vec = [&](const char* name, int len) {
        snprintf(e[n].name, sizeof(e[n].name), "%s", name);
        e[n].offset = off; e[n].rows = len; e[n].cols = 0; off += len; ++n;
    };
    auto lin = [&](const char* name, int rows, int cols) {
        snprintf(e[n].name, sizeof(e[n].name), "%s.weight", name);
        e[n].offset = off; e[n].rows = rows; e[n].cols = cols; off += (int64_t)rows * cols; ++n;
        snprintf(e[n].name, sizeof(e[n].name), "%s.bias", name);
        e[n].offset = off; e[n].rows = rows; e[n].cols = 0; off += rows; ++n;
    };
    snprintf(e[n].name, sizeof(e[n].name), "theta");
    e[n].offset = off; e[n].rows = 1; e[n].cols = 1; off += 1; ++n;
    if (no >= 1 && no <= 3) vec("sigma", 1);
    if (no >= 4 && no <= 6) vec("sigma_diag", H);
    lin("initial_network", H, C);
    lin("linear_in", HH, (io >= 3) ? H + 2 : H);
    if (io == 2 || io == 4 || io == 6) lin("emb", H, 2 * H);
    for (int i = 0; i < m->num_hidden_layers - 1; ++i) {
        char nm[32];
        snprintf(nm, sizeof(nm), "linears.%d", i);
        lin(nm, HH, HH);
    }
    lin("linear_out", H, HH);
    if (no == 12 || no == 13) lin("noise_t", H, 2);
    if (no == 14 || no == 15) lin("noise_y", H, H + 2);
    if (no == 16 || no == 17) { lin("noise_t.0", H, 2); lin("noise_t.2", H, H); }
    if (no == 18 || no == 19) { lin("noise_y.0", H, H + 2); lin("noise_y.2", H, H); }
    *count = n;
    *total = off;
    return SNSDE_OK;
}

int find(const ParamEntry* e, int n, const char* name) {
    for (int i = 0; i < n; ++i)
        if (strcmp(e[i].name, name) == 0) return i;
    return -1;
}

}  // namespace

int snsde_build_net(const snsde_model& m, int32_t n_steps, SnsdeNet* net) {
    ParamEntry e[MAX_PARAMS];
    int n = 0;
    int64_t total = 0;
    int rc = build_params(&m, e, &n, &total);
    if (rc) return rc;
    if (total > 0x7fffffffLL) return SNSDE_ERR_DIMS;
    memset(net, 0, sizeof(*net));
    const int io = m.input_option, no = m.noise_option;
    int32_t woff = 0;
    auto fill = [&](SnsdeLayer& L, const char* name, int tshift, bool packed) {
        char w[48], b[48];
        snprintf(w, sizeof(w), "%s.weight", name);
        snprintf(b, sizeof(b), "%s.bias", name);
        const int iw = find(e, n, w), ib = find(e, n, b);
        if (iw < 0) { L.present = 0; L.w = -1; return; }
        L.present = 1;
        L.src_w = (int32_t)e[iw].offset;
        L.src_b = (int32_t)e[ib].offset;
        L.N = e[iw].rows;
        L.K = e[iw].cols;
        L.Kpad = (L.K + 3) & ~3;
        L.tshift = tshift;
        if (packed) { L.w = woff; woff += L.Kpad * L.N; } else { L.w = -1; }
    };
    const bool uses_x = (io == 0 || io == 2 || io == 4 || io == 6);
    fill(net->init, "initial_network", 0, uses_x);
    if (!uses_x) net->init.w = -1;
    fill(net->in, "linear_in", io >= 3 ? 2 : 0, io != 0);
    if (io == 0) net->in.w = -1;
    fill(net->emb, "emb", 0, true);
    net->n_hid = m.num_hidden_layers - 1;
    for (int i = 0; i < net->n_hid; ++i) {
        char nm[32];
        snprintf(nm, sizeof(nm), "linears.%d", i);
        fill(net->hid[i], nm, 0, true);
    }
    fill(net->out, "linear_out", 0, true);
    if (no == 14 || no == 15) fill(net->ny0, "noise_y", 2, true);
    if (no == 18 || no == 19) { fill(net->ny0, "noise_y.0", 2, true); fill(net->ny1, "noise_y.2", 0, true); }
    if (no == 12 || no == 13) fill(net->nt0, "noise_t", 0, false);
    if (no == 16 || no == 17) { fill(net->nt0, "noise_t.0", 0, false); fill(net->nt1, "noise_t.2", 0, false); }
    net->off_theta = (int32_t)e[find(e, n, "theta")].offset;
    int i = find(e, n, "sigma");
    net->off_sigma = i >= 0 ? (int32_t)e[i].offset : -1;
    i = find(e, n, "sigma_diag");
    net->off_sigma_diag = i >= 0 ? (int32_t)e[i].offset : -1;
    net->packed_floats = (woff + 3) & ~3;
    net->gt_tab = (no == 12 || no == 13 || no == 16 || no == 17) ? net->packed_floats : -1;
    (void)n_steps;
    return SNSDE_OK;
}

// global_rows (snsde.h): 0, or the rows of the whole problem - this shard's rows row_offset .. row_offset + batch - 1 lie inside it
static bool global_rows_ok(const snsde_solve* s) {
    return s->global_rows == 0 || (s->global_rows > 0 && s->row_offset >= 0 && s->global_rows - s->row_offset >= (int64_t)s->batch);
}

// row_offset (snsde.h): the first Philox counter word is the global row as a uint32 - every row of the call lies in [0, 2^32),
// with or without global_rows (a row beyond it would silently draw the Brownian path of row - 2^32)
static bool row_range_ok(const snsde_solve* s) {
    return s->row_offset >= 0 && s->row_offset <= ((int64_t)1 << 32) - (int64_t)s->batch;
}

// samples (snsde.h): S paths per input row - whole groups of S paths per call, shard and problem
static bool samples_ok(const snsde_solve* s) {
    if (s->samples < 0 || s->reserved3 != 0) return false;
    const int64_t S = snsde_samples(s);
    return S == 1 || (s->batch % S == 0 && s->row_offset % S == 0 && s->global_rows % S == 0);
}
// SNSDE_FLAG_SAMPLE_GRAD (snsde.h): the opt-in to training through the sample paths; nothing without samples > 1
static bool sample_grad(const snsde_solve* s) { return snsde_samples(s) > 1 && (s->flags & SNSDE_FLAG_SAMPLE_GRAD) != 0; }
// SNSDE_FLAG_BF16_GRAD (snsde.h): the opt-in to training through the bf16-operand forward; nothing without bf16 operands
static bool bf16_grad(const snsde_solve* s) {
    return (s->flags & SNSDE_FLAG_BF16_OPERANDS) != 0 && (s->flags & SNSDE_FLAG_BF16_GRAD) != 0;
}
static bool samples_training(const snsde_solve* s) {
    return snsde_samples(s) > 1 && (s->act_save || s->stage_save || s->traj || s->dW_out || s->dU_out);
}
// ... an inference-only solve: no training-mode planes unless the flag opts in (never together with bf16 operands), and the
// initial state is the caller's (one row per path) either way
static bool samples_inference_only(const snsde_solve* s) {
    if (sample_grad(s) && (s->flags & SNSDE_FLAG_BF16_OPERANDS)) return false;
    return !(samples_training(s) && !sample_grad(s)) && !(snsde_samples(s) > 1 && s->z0_weight);
}

// ... and the forward plans whose training planes the sampled adjoint route takes (route_backward): the lean kernel and the general
// MFMA kernel, elementwise diffusions, H <= 128 - the planes of any other plan would have no backward to read them
static bool sampled_training_plan(const snsde_mfma::MfmaPlan& p) {
    return p.ok && p.H != 256 && p.NN == 0 && (p.kernel == snsde_mfma::FwdKernel::lean || p.kernel == snsde_mfma::FwdKernel::general_m4 ||
                                               p.kernel == snsde_mfma::FwdKernel::general_m16);
}

// SNSDE_FLAG_ENSEMBLE_SAMPLES (snsde.h): the opt-in to sample paths of a model ensemble; nothing without members > 1 and samples > 1
static bool ensemble_samples(const snsde_solve* s) {
    return snsde_members(s) > 1 && snsde_samples(s) > 1 && (s->flags & SNSDE_FLAG_ENSEMBLE_SAMPLES) != 0;
}
// members (snsde.h): M models in one call - whole members, each a whole number of 4-row tiles and, with sample paths under
// SNSDE_FLAG_ENSEMBLE_SAMPLES, of sample groups (a group never straddles two members)
static bool members_ok(const snsde_solve* s) {
    if (s->members < 0) return false;
    const int32_t M = snsde_members(s);
    if (M == 1) return true;
    if (s->batch % M != 0 || (s->batch / M) % 4 != 0) return false;
    return !ensemble_samples(s) || (s->batch / M) % snsde_samples(s) == 0;
}
// SNSDE_FLAG_ENSEMBLE_GRAD (snsde.h): the opt-in to training through a model ensemble; nothing without members > 1
static bool ensemble_grad(const snsde_solve* s) { return snsde_members(s) > 1 && (s->flags & SNSDE_FLAG_ENSEMBLE_GRAD) != 0; }
static bool members_training(const snsde_solve* s) {
    return snsde_members(s) > 1 && (s->act_save || s->stage_save || s->traj || s->dW_out || s->dU_out);
}
// ... an inference-only solve of the members' own fields from the caller's initial states: not combined with sample paths (unless
// SNSDE_FLAG_ENSEMBLE_SAMPLES opts in), a fused initial network, a supplied diffusion table (one table, M models), the accumulator
// column or - unless the flag opts in - any training-mode plane
static bool members_refused(const snsde_solve* s) {
    return snsde_members(s) > 1 && ((snsde_samples(s) > 1 && !ensemble_samples(s)) || s->z0_weight || s->noise_table || s->kl_column1 != 0 ||
                                    (members_training(s) && !ensemble_grad(s)));
}
// ... and the forward plans whose training planes the ensemble adjoint route takes (route_backward): the lean kernel and the general
// MFMA kernel on 4-row tiles, elementwise diffusions, H <= 128
// SNSDE_FLAG_ENSEMBLE_NETS_GRAD (snsde.h) adds the wave pairs - with all three of ENSEMBLE_NETS | ENSEMBLE_GRAD | ENSEMBLE_NETS_GRAD
// set, nothing otherwise - whose adjoints carry the member on their second grid axis (snsde_w4_kernel.h: ENS)
static bool ensemble_nets_grad(const snsde_solve* s) {
    constexpr uint32_t all = SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_GRAD | SNSDE_FLAG_ENSEMBLE_NETS_GRAD;
    return snsde_members(s) > 1 && (s->flags & all) == all;
}
static bool ensemble_training_plan(const snsde_solve* s, const snsde_mfma::MfmaPlan& p) {
    if (p.ok && p.kernel == snsde_mfma::FwdKernel::w4) return ensemble_nets_grad(s) && snsde_samples(s) <= 1;
    return p.ok && p.H <= 128 && p.NN == 0 && (p.kernel == snsde_mfma::FwdKernel::lean || p.kernel == snsde_mfma::FwdKernel::general_m4);
}
// One member of an ensemble run alone as a shard of the whole (snsde.h: members): what each member is planned as - its adjoint's
// workgroups and partial-sum blocks, its weight-gradient tiles and splits.  (row_offset: member 0's; no plan reads it.)  `samples`
// stays: under SNSDE_FLAG_ENSEMBLE_SAMPLES the member alone is a sampled solve of its batch / M paths
static snsde_solve member_alone(const snsde_solve* s) {
    snsde_solve one = *s;
    one.batch = s->batch / snsde_members(s);
    one.global_rows = snsde_plan_rows(s);
    one.members = 0;
    return one;
}

int snsde_flavor_hint(const snsde_solve* s) {
    if (snsde_solve_variant(s)) return 1;      // tutorial-style fields: 4-row tiles only
    return s->kernel == SNSDE_KERNEL_MFMA_M16 ? 0 : (s->kernel == SNSDE_KERNEL_MFMA_M4 ? 1 : (s->kernel == SNSDE_KERNEL_MFMA_W4 ? 2 : -1));
}

// Which kernel runs the forward solve of a descriptor (SNSDE_PATH_*): the one decision behind snsde_solve_forward and
// snsde_forward_path.  An MFMA path carries the plan snsde_mfma_launch runs (the plan names the kernel).
struct ForwardRoute { int path; snsde_mfma::MfmaPlan plan; };

static ForwardRoute route_forward(const snsde_solve* s, const SnsdeNet& net) {
    ForwardRoute r{};      // (SNSDE_PATH_NONE)
    const int k = s->kernel;
    const bool variant = snsde_solve_variant(s);
    const int generic = s->method == SNSDE_SRK ? SNSDE_PATH_GENERIC_SRK : SNSDE_PATH_GENERIC;
    if (k < SNSDE_KERNEL_AUTO || k > SNSDE_KERNEL_MFMA_W4) return r;
    if (!samples_ok(s) || !samples_inference_only(s)) return r;
    // model ensembles: the MFMA kernels that map a tile to its member, or nothing - the generic family is neither a request nor a fallback
    const bool ensemble = snsde_members(s) > 1;
    if (!members_ok(s) || members_refused(s) || (ensemble && k == SNSDE_KERNEL_GENERIC)) return r;
    if (variant && (k == SNSDE_KERNEL_GENERIC || k == SNSDE_KERNEL_MFMA_M16)) return r;   // tutorial-style fields: 4-row tiles or nothing
    // training planes of a sampled solve (SNSDE_FLAG_SAMPLE_GRAD): the MFMA kernels the sampled adjoint route covers, or nothing
    const bool strain = samples_training(s);
    if (strain && (variant || s->kl_column1 != 0)) return r;
    // training planes of an ensemble (SNSDE_FLAG_ENSEMBLE_GRAD): the kernels the ensemble adjoint route covers, or nothing
    const bool etrain = members_training(s);
    if (etrain && (variant || (s->flags & SNSDE_FLAG_BF16_OPERANDS))) return r;
    if (k == SNSDE_KERNEL_GENERIC) { if (!(s->flags & SNSDE_FLAG_BF16_OPERANDS) && !strain) r.path = generic; return r; }
    if (!global_rows_ok(s)) return r;
    r.plan = make_plan(s, net, snsde_flavor_hint(s));
    if (strain && !sampled_training_plan(r.plan)) return ForwardRoute{};
    if (etrain && !ensemble_training_plan(s, r.plan)) return ForwardRoute{};
    // `auto` falls back to the generic family (SRK: its SRK variant) where no MFMA kernel takes the descriptor - but not where the
    // plan made for the whole problem (global_rows) names a kernel this shard cannot run, nor where the plan arrives at a kernel
    // that does not address coeffs by sample group (samples): that is no kernel at all
    r.path = r.plan.ok ? snsde_mfma_path(r.plan)
                       : (k == SNSDE_KERNEL_AUTO && !variant && !r.plan.shard_refused && !r.plan.samples_refused && !ensemble ? generic
                                                                                                                             : SNSDE_PATH_NONE);
    // bf16 operands: the bf16 lean kernel or nothing (no f32 kernel stands in for it)
    if ((s->flags & SNSDE_FLAG_BF16_OPERANDS) && r.path != SNSDE_PATH_LEAN_BF16) r = ForwardRoute{};
    return r;
}

// The adjoint of a descriptor: the one decision behind every backward entry point (snsde_mfma_kernels.h: BackwardRoute).  Both plans
// are made here, once, with the forward launch's flavour hint, and handed down: the launchers do not plan.
// mode 1: MFMA adjoint kernel (forward on the MFMA path with act_save); 2: generic adjoint kernel (forward on the generic kernel,
// traj + dW_out only); 0: no fused backward for this configuration
static snsde_mfma::BackwardRoute route_backward(const snsde_solve* s, const SnsdeNet& net) {
    snsde_mfma::BackwardRoute r{};
    const int hint = snsde_flavor_hint(s), k = s->kernel;
    if (!global_rows_ok(s)) return r;
    if (!members_ok(s)) return r;
    if (snsde_members(s) > 1) {
        // model ensembles: an inference-only forward, no adjoint and nothing to plan - unless SNSDE_FLAG_ENSEMBLE_GRAD opts in.  Then
        // mode 1 exactly where the forward plan is the lean or the general kernel on 4-row tiles (make_plan refuses the others) and the
        // adjoint of ONE member run alone as a shard of the whole is the general MFMA adjoint on 4-row tiles or its SRK form, which
        // read no coefficients and leave delta planes.  Under SNSDE_FLAG_ENSEMBLE_NETS_GRAD (ensemble_nets_grad) also where the
        // forward plan is the wave pairs and the member alone takes the wave-pair adjoint with the weight gradients inside (Euler or
        // SRK; never its delta-plane variant): each block of the backward workspace then also holds that member's per-tile gradient
        // blocks (RevPlan::w4_gpart_off).  Anything else is no plan (never another kernel, no mode 2)
        // Sample paths of the ensemble (SNSDE_FLAG_ENSEMBLE_SAMPLES, else refused): SNSDE_FLAG_SAMPLE_GRAD as well - the member alone
        // is then planned as a sampled solve, whose adjoint route asks for these same two adjoints
        if (!samples_ok(s) || (snsde_samples(s) > 1 && !sample_grad(s))) return r;
        if (!ensemble_grad(s) || members_refused(s) || (s->flags & SNSDE_FLAG_BF16_OPERANDS) || snsde_solve_variant(s) ||
            k == SNSDE_KERNEL_GENERIC || k == SNSDE_KERNEL_MFMA_M16 || (s->method == SNSDE_MILSTEIN && s->model.noise_option == 7) ||
            (s->method != SNSDE_EULER && s->method != SNSDE_MILSTEIN && s->method != SNSDE_SRK))
            return r;
        const snsde_solve one = member_alone(s);
        r.fp = make_plan(s, net, hint);
        if (!ensemble_training_plan(s, r.fp)) return snsde_mfma::BackwardRoute{};
        r.rp = make_rev_plan(&one, net, r.fp, hint);
        const bool pairs = r.fp.kernel == snsde_mfma::FwdKernel::w4;
        if (!r.rp.ok || r.rp.FL != 1 ||
            (pairs ? r.rp.kernel != snsde_mfma::RevKernel::w4_fused || (s->method != SNSDE_EULER && s->method != SNSDE_SRK)
                   : (r.rp.kernel != snsde_mfma::RevKernel::general && r.rp.kernel != snsde_mfma::RevKernel::general_srk)))
            return snsde_mfma::BackwardRoute{};
        r.members = snsde_members(s);
        size_t g = 0;
        snsde_generic_workspace_floats(&one, net, &g);
        r.bws_stride = snsde_member_bws_stride((r.rp.workspace_floats > g ? r.rp.workspace_floats : g) + 64);      // (as backward_workspace_bytes sizes one model)
        r.fws_stride = snsde_member_ws_stride(s, net);
        if (r.fws_stride == 0) return snsde_mfma::BackwardRoute{};
        r.mode = 1;
        return r;
    }
    const bool sampled = snsde_samples(s) > 1;
    // sample paths: an inference-only forward, no adjoint and nothing to plan - unless SNSDE_FLAG_SAMPLE_GRAD opts in
    if ((sampled && (!sample_grad(s) || (s->flags & SNSDE_FLAG_BF16_OPERANDS))) || !samples_ok(s)) return r;
    r.fp = make_plan(s, net, hint);
    r.rp = make_rev_plan(s, net, r.fp, hint);
    if (sampled) {
        // the sampled adjoint route: a forward kernel that maps path p to coeffs row p / S (make_plan refuses the others) and the
        // general MFMA adjoint, which reads no coefficients and leaves delta planes - the weight-gradient pass and
        // snsde_coeff_gradients map paths to input rows themselves.  Anything else is no plan (never another kernel, no mode 2)
        const bool fwd_ok = sampled_training_plan(r.fp);
        const bool rev_ok = r.rp.ok && (r.rp.kernel == snsde_mfma::RevKernel::general || r.rp.kernel == snsde_mfma::RevKernel::general_srk);
        if (!fwd_ok || !rev_ok || s->kl_column1 != 0 || snsde_solve_variant(s) || k == SNSDE_KERNEL_GENERIC ||
            (s->method == SNSDE_MILSTEIN && s->model.noise_option == 7))
            return snsde_mfma::BackwardRoute{};
        r.mode = 1;
        return r;
    }
    if (s->flags & SNSDE_FLAG_BF16_OPERANDS) {
        // an inference-only forward: no adjoint of any kind - unless SNSDE_FLAG_BF16_GRAD opts in.  Then mode 1 exactly where the
        // forward plan is the bf16 lean kernel and the adjoint make_rev_plan gives that lean forward is the general one, which leaves
        // delta planes (its pack rounds the transposed weights, the weight-gradient pass its X operands); a supplied noise_table
        // and everything the forward plan refuses (SRK, nets, other H, field variants, kl_column1) is no plan: never an f32 kernel,
        // never mode 2
        if (bf16_grad(s) && r.fp.ok && r.fp.kernel == snsde_mfma::FwdKernel::lean_bf16 && r.rp.ok &&
            r.rp.kernel == snsde_mfma::RevKernel::general && !s->noise_table && s->kl_column1 == 0 && !snsde_solve_variant(s) &&
            k != SNSDE_KERNEL_GENERIC && k != SNSDE_KERNEL_MFMA_M16)
            r.mode = 1;
        return r;
    }
    if (r.fp.shard_refused) return r;                      // (no forward kernel either: route_forward)
    if (s->method == SNSDE_MILSTEIN && s->model.noise_option == 7) return r;     // no forward kernel either (validate_solve)
    const bool variant = snsde_solve_variant(s);      // tutorial-style fields: the 4-row-tile MFMA adjoint or nothing
    if (r.rp.ok && k != SNSDE_KERNEL_GENERIC && !(variant && k == SNSDE_KERNEL_MFMA_M16)) r.mode = 1;
    else if (!variant && snsde_generic_backward_supported(s)) r.mode = 2;
    return r;
}

// (the generic adjoints pack their own weights / tables)
static size_t backward_workspace_bytes(const snsde_backward* b, const SnsdeNet& net, const snsde_mfma::BackwardRoute& r) {
    if (r.members > 1) return (size_t)r.members * r.bws_stride * sizeof(float);      // (one block per member: snsde_member_bws_stride)
    size_t f = r.rp.ok ? r.rp.workspace_floats : 0, g = 0;
    snsde_generic_workspace_floats(&b->fwd, net, &g);
    return ((f > g ? f : g) + 64) * sizeof(float);
}

extern "C" {

int snsde_version(void) { return SNSDE_VERSION; }

int snsde_abi_check(int version, size_t sizeof_model, size_t sizeof_solve, size_t sizeof_backward, size_t sizeof_head) {
    // 0 = "this binding does not declare that struct" (a forward-only binding has no snsde_backward / snsde_head)
    auto same = [](size_t got, size_t want) { return got == 0 || got == want; };
    return (version == SNSDE_VERSION && same(sizeof_model, sizeof(snsde_model)) && same(sizeof_solve, sizeof(snsde_solve)) &&
            same(sizeof_backward, sizeof(snsde_backward)) && same(sizeof_head, sizeof(snsde_head))) ? SNSDE_OK : SNSDE_ERR_ABI;
}

const char* snsde_strerror(int code) {
    switch (code) {
        case SNSDE_OK: return "ok";
        case SNSDE_ERR_NULL: return "required pointer is NULL";
        case SNSDE_ERR_DIMS: return "bad or inconsistent dimensions";
        case SNSDE_ERR_OPTION: return "input_option must be 0..6 and noise_option 0..19";
        case SNSDE_ERR_UNSUPPORTED: return "configuration not supported by this build";
        case SNSDE_ERR_WORKSPACE: return "workspace too small";
        case SNSDE_ERR_LDS: return "configuration exceeds the LDS budget";
        case SNSDE_ERR_TS: return "ts must be strictly increasing, dt > 0 and representable progress in float32";
        case SNSDE_ERR_LAUNCH: return "HIP kernel launch failed";
        case SNSDE_ERR_INDEX: return "index out of range";
        case SNSDE_ERR_ABI: return "struct_size / version mismatch: the binding was built against another include/snsde.h";
        default: return "unknown error";
    }
}

int snsde_param_count(const snsde_model* m) {
    ParamEntry e[MAX_PARAMS];
    int n = 0;
    int64_t total = 0;
    int rc = build_params(m, e, &n, &total);
    return rc ? rc : n;
}

int64_t snsde_param_numel(const snsde_model* m) {
    ParamEntry e[MAX_PARAMS];
    int n = 0;
    int64_t total = 0;
    int rc = build_params(m, e, &n, &total);
    return rc ? rc : total;
}

int snsde_param_info(const snsde_model* m, int index, char* name, int name_cap, int64_t* offset, int32_t* rows,
                     int32_t* cols) {
    ParamEntry e[MAX_PARAMS];
    int n = 0;
    int64_t total = 0;
    int rc = build_params(m, e, &n, &total);
    if (rc) return rc;
    if (index < 0 || index >= n) return SNSDE_ERR_INDEX;
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", e[index].name);
    if (offset) *offset = e[index].offset;
    if (rows) *rows = e[index].rows;
    if (cols) *cols = e[index].cols;
    return SNSDE_OK;
}

// torchsde 0.2.5 BaseSDESolver.integrate time bookkeeping in float32.
static int walk_grid(const float* ts, int32_t T, double dt, const float* times, int32_t L, int32_t cap,
                     float* step_tab, int32_t* out_step, float* out_w, int32_t* n_steps) {
    if (!ts) return SNSDE_ERR_NULL;
    if (T < 2) return SNSDE_ERR_TS;
    if (!(dt > 0)) return SNSDE_ERR_TS;
    for (int k = 1; k < T; ++k)
        if (!(ts[k] > ts[k - 1])) return SNSDE_ERR_TS;
    const float step = (float)dt;
    const float t_end = ts[T - 1];
    float curr = ts[0], prev = ts[0];
    int32_t n = 0;
    for (int k = 1; k < T; ++k) {
        const float out_t = ts[k];
        while (curr < out_t) {
            volatile float nx = curr + step;  // force fp32 rounding
            float nxt = nx;
            if (t_end < nxt) nxt = t_end;
            if (!(nxt > curr)) return SNSDE_ERR_TS;
            if (step_tab) {
                if (n >= cap) return SNSDE_ERR_DIMS;
                float* r = step_tab + (size_t)n * SNSDE_STEP_STRIDE;
                volatile float h = nxt - curr;
                r[0] = curr;
                r[1] = h;
                r[2] = sinf(curr);
                r[3] = cosf(curr);
                int idx = 0;
                if (times) {
                    int cnt = 0;
                    for (int j = 0; j < L; ++j) cnt += (curr > times[j]) ? 1 : 0;
                    idx = cnt - 1;
                    if (idx < 0) idx = 0;
                    if (idx > L - 2) idx = L - 2;
                    volatile float fr = curr - times[idx];
                    r[4] = fr;
                } else {
                    r[4] = 0.0f;
                }
                memcpy(&r[5], &idx, sizeof(float));
                r[6] = sqrtf(h);
                r[7] = nxt;
                r[8] = r[9] = r[10] = r[11] = 0.0f;
            }
            prev = curr;
            curr = nxt;
            ++n;
        }
        if (out_step) {
            out_step[k - 1] = n - 1;
            if (step_tab) {   // per-step output bookkeeping: count and first output index
                float* r = step_tab + (size_t)(n - 1) * SNSDE_STEP_STRIDE;
                int32_t cnt, first;
                memcpy(&cnt, &r[8], 4);
                memcpy(&first, &r[9], 4);
                if (cnt == 0) first = k - 1;
                ++cnt;
                memcpy(&r[8], &cnt, 4);
                memcpy(&r[9], &first, 4);
            }
            volatile float denom = curr - prev;
            volatile float a = curr - out_t, b = out_t - prev;
            out_w[2 * (k - 1)] = a / denom;
            out_w[2 * (k - 1) + 1] = b / denom;
        }
    }
    *n_steps = n;
    return SNSDE_OK;
}

int snsde_grid_count(const float* ts, int32_t n_out, double dt, int32_t* n_steps) {
    if (!n_steps) return SNSDE_ERR_NULL;
    return walk_grid(ts, n_out, dt, nullptr, 0, 0, nullptr, nullptr, nullptr, n_steps);
}

int snsde_grid_build(const float* ts, int32_t n_out, double dt, const float* times, int32_t knots, int32_t n_steps,
                     float* step_tab, int32_t* out_step, float* out_w) {
    if (!step_tab || !out_step || !out_w || !times) return SNSDE_ERR_NULL;
    if (knots < 2) return SNSDE_ERR_DIMS;
    int32_t n = 0;
    int rc = walk_grid(ts, n_out, dt, times, knots, n_steps, step_tab, out_step, out_w, &n);
    if (rc) return rc;
    return n == n_steps ? SNSDE_OK : SNSDE_ERR_DIMS;
}

int snsde_grid_srk_build(const float* step_tab, int32_t n_steps, const float* times, int32_t knots, float* srk_tab) {
    if (!step_tab || !times || !srk_tab) return SNSDE_ERR_NULL;
    if (n_steps <= 0 || knots < 2) return SNSDE_ERR_DIMS;
    const float cs[4] = {0.0f, 0.25f, 0.5f, 1.0f};
    for (int n = 0; n < n_steps; ++n) {
        const float t0 = step_tab[(size_t)n * SNSDE_STEP_STRIDE], h = step_tab[(size_t)n * SNSDE_STEP_STRIDE + 1];
        for (int c = 0; c < 4; ++c) {
            volatile float ch = cs[c] * h;
            volatile float t = t0 + ch;
            float* r = srk_tab + ((size_t)n * 4 + c) * SNSDE_SRK_STRIDE;
            int cnt = 0;
            for (int j = 0; j < knots; ++j) cnt += (t > times[j]) ? 1 : 0;
            int idx = cnt - 1;
            if (idx < 0) idx = 0;
            if (idx > knots - 2) idx = knots - 2;
            volatile float fr = t - times[idx];
            r[0] = t; r[1] = sinf(t); r[2] = cosf(t); r[3] = fr;
            memcpy(&r[4], &idx, sizeof(float));
            r[5] = r[6] = r[7] = 0.0f;
        }
    }
    return SNSDE_OK;
}

static int validate_solve(const snsde_solve* s, bool eval) {
    if (!s) return SNSDE_ERR_NULL;
    if (s->struct_size != sizeof(snsde_solve)) return SNSDE_ERR_ABI;      // stale binding: refuse before reading any field
    int rc = validate_model(&s->model);
    if (rc) return rc;
    if (s->batch <= 0 || s->knots < 2) return SNSDE_ERR_DIMS;
    if (!row_range_ok(s) || !global_rows_ok(s) || !samples_ok(s) || !members_ok(s)) return SNSDE_ERR_DIMS;
    if (!s->params || !s->coeffs || !s->workspace) return SNSDE_ERR_NULL;
    if (!eval) {
        if (s->n_steps <= 0 || s->n_out < 2) return SNSDE_ERR_DIMS;
        if (!s->step_tab || !s->out_step || !s->out_w || !s->y0 || !s->ys) return SNSDE_ERR_NULL;
        if (s->method != SNSDE_EULER && s->method != SNSDE_MILSTEIN && s->method != SNSDE_SRK) return SNSDE_ERR_OPTION;
        if (s->method == SNSDE_SRK && !s->srk_tab) return SNSDE_ERR_NULL;
        if (s->method == SNSDE_SRK && s->dW && !s->dU) return SNSDE_ERR_NULL;   // supplied dW needs its Levy integral
        const int no = s->model.noise_option;
        // Milstein: g dg/dy in closed form where g_i depends on y through y_i only, a transposed pass through the
        // diffusion net for 14/15/18/19 (generic kernels); sqrt(y) has no finite derivative at the clipped values
        if (s->method == SNSDE_MILSTEIN && no == 7) return SNSDE_ERR_UNSUPPORTED;
        if (s->noise_table && no != 12 && no != 13) return SNSDE_ERR_OPTION;   // a supplied table is the time-only factor
        if ((s->z0_weight != nullptr) != (s->z0_bias != nullptr)) return SNSDE_ERR_NULL;
        if (s->kl_column1 < 0 || s->kl_column1 > s->model.hidden_channels || s->reserved2 != 0) return SNSDE_ERR_DIMS;
        if (!samples_inference_only(s)) return SNSDE_ERR_UNSUPPORTED;
        if (members_refused(s)) return SNSDE_ERR_UNSUPPORTED;
    }
    return SNSDE_OK;
}

size_t snsde_workspace_bytes(const snsde_solve* s) {
    if (!s || s->struct_size != sizeof(snsde_solve)) return 0;
    SnsdeNet net;
    if (snsde_build_net(s->model, s->n_steps, &net)) return 0;
    size_t f = 0;
    snsde_solve tmp = *s;
    if (tmp.n_steps < 1) tmp.n_steps = 1;
    tmp.samples = 0;      // (the workspace holds weights and tables: nothing per sample, and no plan is refused for the query)
    tmp.members = 0;
    // model ensembles: one prepared block per member (snsde_member_ws_stride); where no MFMA kernel plans the model there is no
    // ensemble launch either, and the query answers as for one model
    if (const size_t stride = snsde_members(s) > 1 ? snsde_member_ws_stride(&tmp, net) : 0) return (size_t)snsde_members(s) * stride * sizeof(float);
    snsde_generic_workspace_floats(&tmp, net, &f);
    const size_t fm = snsde_mfma_workspace_floats(&tmp, net);
    if (fm > f) f = fm;
    return (f + 64) * sizeof(float);
}

// One launch path for both forward entry points: step_offset = n0 is a stream coordinate (like row_offset and seed), not a plan input -
// route_forward never sees it; the kernels add it to the local step index at their Philox sites only (include/snsde.h).
int snsde_solve_forward_at(const snsde_solve* s, int64_t step_offset, void* hip_stream) {
    int rc = validate_solve(s, false);
    if (rc) return rc;
    if (s->kernel < SNSDE_KERNEL_AUTO || s->kernel > SNSDE_KERNEL_MFMA_W4) return SNSDE_ERR_OPTION;
    if (step_offset < 0 || step_offset + (int64_t)s->n_steps > (int64_t)INT32_MAX) return SNSDE_ERR_DIMS;
    // a continued solve starts from the caller's state, and has a backward under SNSDE_FLAG_RESUME_GRAD only (the _at backward calls)
    if (step_offset != 0 && (((s->act_save || s->stage_save) && !(s->flags & SNSDE_FLAG_RESUME_GRAD)) || s->z0_weight)) return SNSDE_ERR_UNSUPPORTED;
    if (s->workspace_bytes < snsde_workspace_bytes(s)) return SNSDE_ERR_WORKSPACE;
    SnsdeNet net;
    rc = snsde_build_net(s->model, s->n_steps, &net);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int n0 = (int)step_offset;
    const ForwardRoute r = route_forward(s, net);
    if (r.path == SNSDE_PATH_NONE) return SNSDE_ERR_UNSUPPORTED;
    if (r.plan.ok) return snsde_mfma_launch(s, net, r.plan, st, n0);
    if (s->z0_weight && (rc = snsde_z0_launch(s, st)) != SNSDE_OK) return rc;
    if (r.path == SNSDE_PATH_GENERIC_SRK) return snsde_srk_launch(s, net, st, n0);
    return snsde_generic_launch(s, net, st, 0, nullptr, nullptr, nullptr, nullptr, n0);
}

int snsde_solve_forward(const snsde_solve* s, void* hip_stream) { return snsde_solve_forward_at(s, 0, hip_stream); }

int snsde_initial_state(const snsde_solve* s, void* hip_stream) {
    if (!s) return SNSDE_ERR_NULL;
    if (s->struct_size != sizeof(snsde_solve)) return SNSDE_ERR_ABI;
    if (s->batch <= 0 || s->knots < 2 || s->model.hidden_channels <= 0 || s->model.input_channels <= 0) return SNSDE_ERR_DIMS;
    if ((int64_t)s->batch * s->model.hidden_channels > INT32_MAX) return SNSDE_ERR_DIMS;      // (the launch counts elements in 32 bits)
    if (!s->coeffs) return SNSDE_ERR_NULL;
    return snsde_z0_launch(s, static_cast<hipStream_t>(hip_stream));      // (SNSDE_ERR_NULL without z0_weight, z0_bias, y0 or step_tab)
}

// Host-only query: the kernel family snsde_solve_forward would launch for this descriptor (needs model, batch, knots,
// n_steps, method, kernel, flags, input dims; no device pointers).  SNSDE_PATH_NONE = no kernel covers the request
// (snsde_solve_forward returns SNSDE_ERR_UNSUPPORTED and the host layer takes its tensor loop).
int snsde_forward_path(const snsde_solve* s) {
    if (!s || s->struct_size != sizeof(snsde_solve) || validate_model(&s->model) || s->batch <= 0 || s->knots < 2 || s->n_steps <= 0) return SNSDE_PATH_NONE;
    if (s->method == SNSDE_MILSTEIN && s->model.noise_option == 7) return SNSDE_PATH_NONE;
    SnsdeNet net;
    if (snsde_build_net(s->model, s->n_steps, &net)) return SNSDE_PATH_NONE;
    return route_forward(s, net).path;
}

int snsde_lean_variant(const snsde_solve* s) {
    if (snsde_forward_path(s) != SNSDE_PATH_LEAN) return SNSDE_LEAN_NONE;
    SnsdeNet net;
    if (snsde_build_net(s->model, s->n_steps, &net)) return SNSDE_LEAN_NONE;
    const ForwardRoute r = route_forward(s, net);
    if (r.plan.kernel != snsde_mfma::FwdKernel::lean) return SNSDE_LEAN_NONE;
    return r.plan.LEAN_SPEC ? SNSDE_LEAN_SPECIALISED : SNSDE_LEAN_GENERAL;
}

// The kernel the forward route names (SNSDE_FWD_*): the plan's FwdKernel on an MFMA route, the generic family's two launchers otherwise
static int forward_kernel_of(const ForwardRoute& r) {
    using snsde_mfma::FwdKernel;
    if (r.path == SNSDE_PATH_NONE) return SNSDE_FWD_NONE;
    if (!r.plan.ok) return r.path == SNSDE_PATH_GENERIC_SRK ? SNSDE_FWD_GENERIC_SRK : SNSDE_FWD_GENERIC;
    switch (r.plan.kernel) {
        case FwdKernel::w4: return SNSDE_FWD_W4;
        case FwdKernel::m4n: return SNSDE_FWD_M4N;
        case FwdKernel::lean: return SNSDE_FWD_LEAN;
        case FwdKernel::lean_two_tile_h128: return SNSDE_FWD_LEAN_TWO_TILE_H128;
        case FwdKernel::lean_two_tile_h256: return SNSDE_FWD_LEAN_TWO_TILE_H256;
        case FwdKernel::lean_streamed_h256: return SNSDE_FWD_LEAN_STREAMED_H256;
        case FwdKernel::general_m4: return SNSDE_FWD_GENERAL_M4;
        case FwdKernel::general_m16: return SNSDE_FWD_GENERAL_M16;
        case FwdKernel::lean_bf16: return SNSDE_FWD_LEAN_BF16;
    }
    return SNSDE_FWD_NONE;
}

int snsde_forward_kernel(const snsde_solve* s, int32_t* nhid, int32_t* kuxt) {
    if (nhid) *nhid = -1;
    if (kuxt) *kuxt = -1;
    if (snsde_forward_path(s) == SNSDE_PATH_NONE) return SNSDE_FWD_NONE;      // (its descriptor checks)
    SnsdeNet net;
    if (snsde_build_net(s->model, s->n_steps, &net)) return SNSDE_FWD_NONE;
    const ForwardRoute r = route_forward(s, net);
    if (r.path != SNSDE_PATH_NONE && r.plan.ok) {
        if (nhid) *nhid = r.plan.NHID;
        if (kuxt) *kuxt = r.plan.KUXT;
    }
    return forward_kernel_of(r);
}

int snsde_backward_kernel(const snsde_solve* s) {
    using snsde_mfma::RevKernel;
    if (snsde_backward_supported(s) == 0) return SNSDE_REV_NONE;      // (its descriptor checks)
    SnsdeNet net;
    if (snsde_build_net(s->model, s->n_steps, &net)) return SNSDE_REV_NONE;
    const snsde_mfma::BackwardRoute r = route_backward(s, net);
    if (r.mode == 2) return SNSDE_REV_GENERIC;
    if (r.mode != 1) return SNSDE_REV_NONE;
    switch (r.rp.kernel) {
        case RevKernel::w4_fused: return SNSDE_REV_W4_FUSED;
        case RevKernel::m4n_srk: return SNSDE_REV_M4N_SRK;
        case RevKernel::m4n_milstein: return SNSDE_REV_M4N_MILSTEIN;
        case RevKernel::general_srk: return SNSDE_REV_GENERAL_SRK;
        case RevKernel::two_tile_h256: return SNSDE_REV_TWO_TILE_H256;
        case RevKernel::general: return SNSDE_REV_GENERAL;
    }
    return SNSDE_REV_NONE;
}

int snsde_eval_fg(const snsde_solve* s, const float* step_row, const float* y, float* f_out, float* g_out,
                  void* hip_stream) {
    int rc = validate_solve(s, true);
    if (rc) return rc;
    if (!step_row || !y || !f_out || !g_out) return SNSDE_ERR_NULL;
    if (snsde_solve_variant(s)) return SNSDE_ERR_UNSUPPORTED;
    if (snsde_samples(s) > 1) return SNSDE_ERR_UNSUPPORTED;      // (the probe is per input row: y and coeffs row for row)
    if (snsde_members(s) > 1) return SNSDE_ERR_UNSUPPORTED;      // (... and of one model)
    snsde_solve tmp = *s;
    tmp.n_steps = 1;
    tmp.n_out = 2;
    tmp.dW = nullptr;
    tmp.traj = nullptr;
    tmp.dW_out = nullptr;
    if (s->workspace_bytes < snsde_workspace_bytes(&tmp)) return SNSDE_ERR_WORKSPACE;
    SnsdeNet net;
    rc = snsde_build_net(s->model, 1, &net);
    if (rc) return rc;
    return snsde_generic_launch(&tmp, net, static_cast<hipStream_t>(hip_stream), 1, y, f_out, g_out, step_row);
}

int snsde_act_slots(const snsde_model* m) {
    int rc = validate_model(m);
    if (rc) return rc;
    // (the per-step count of a one-pass method: snsde_save_layout adds what SRK saves for its fourth evaluation)
    return snsde_save::nsave(m->num_hidden_layers - 1, snsde_noise_net_layers(m->noise_option), SNSDE_EULER, m->activation != SNSDE_ACT_RELU);
}

int snsde_save_layout(const snsde_solve* s, int32_t* act_slots, int32_t* stage_planes, int32_t* delta_slots) {
    if (!s) return SNSDE_ERR_NULL;
    if (s->struct_size != sizeof(snsde_solve)) return SNSDE_ERR_ABI;
    int rc = validate_model(&s->model);
    if (rc) return rc;
    if (!global_rows_ok(s)) return SNSDE_ERR_DIMS;
    const int nhid = s->model.num_hidden_layers - 1, nn = snsde_noise_net_layers(s->model.noise_option);
    const bool smooth = s->model.activation != SNSDE_ACT_RELU;
    const int slots = snsde_save::nsave(nhid, nn, s->method, smooth), planes = snsde_save::stage_planes(nn, s->method);
    if (act_slots) *act_slots = slots;
    if (stage_planes) *stage_planes = planes;
    if (delta_slots) {
        *delta_slots = slots + snsde_save::milstein_slots(nn, s->method);      // (act_save's count + Milstein's factors: snsde_save_layout.h)
        // 0: the adjoint of this solve accumulates the weight gradients itself (wave-pair adjoint, snsde_w4_kernel.h): no delta planes
        SnsdeNet net;
        if (nn > 0 && s->batch > 0 && s->n_steps > 0 && snsde_build_net(s->model, s->n_steps, &net) == SNSDE_OK) {
            const snsde_mfma::BackwardRoute r = route_backward(s, net);
            if (r.mode == 1 && r.rp.kernel == snsde_mfma::RevKernel::w4_fused) *delta_slots = 0;
        }
    }
    return SNSDE_OK;
}

int snsde_backward_supported(const snsde_solve* s) {
    if (!s || s->struct_size != sizeof(snsde_solve) || validate_model(&s->model)) return 0;
    SnsdeNet net;
    if (snsde_build_net(s->model, s->n_steps, &net)) return 0;
    return route_backward(s, net).mode;
}

size_t snsde_backward_workspace_bytes(const snsde_backward* b) {
    if (!b || b->struct_size != sizeof(snsde_backward) || b->fwd.struct_size != sizeof(snsde_solve)) return 0;
    SnsdeNet net;
    if (snsde_build_net(b->fwd.model, b->fwd.n_steps, &net)) return 0;
    return backward_workspace_bytes(b, net, route_backward(&b->fwd, net));
}

// The offset of a backward _at call: the forward's range, and the opt-in a continued training solve needs
static int check_backward_offset(const snsde_solve* s, int64_t step_offset) {
    if (step_offset < 0 || step_offset + (int64_t)s->n_steps > (int64_t)INT32_MAX) return SNSDE_ERR_DIMS;
    if (step_offset != 0 && !(s->flags & SNSDE_FLAG_RESUME_GRAD)) return SNSDE_ERR_UNSUPPORTED;
    return SNSDE_OK;
}

int snsde_solve_backward(const snsde_backward* b, void* hip_stream) { return snsde_solve_backward_at(b, 0, hip_stream); }

int snsde_solve_backward_at(const snsde_backward* b, int64_t step_offset, void* hip_stream) {
    if (!b) return SNSDE_ERR_NULL;
    if (b->struct_size != sizeof(snsde_backward)) return SNSDE_ERR_ABI;
    int rc = validate_solve(&b->fwd, false);
    if (rc) return rc;
    if ((rc = check_backward_offset(&b->fwd, step_offset)) != SNSDE_OK) return rc;
    if ((b->fwd.flags & SNSDE_FLAG_BF16_OPERANDS) && !bf16_grad(&b->fwd)) return SNSDE_ERR_UNSUPPORTED;     // (inference-only forward)
    if (snsde_samples(&b->fwd) > 1 && !sample_grad(&b->fwd)) return SNSDE_ERR_UNSUPPORTED;      // (sample paths: inference only without the opt-in)
    if (snsde_members(&b->fwd) > 1 && !ensemble_grad(&b->fwd)) return SNSDE_ERR_UNSUPPORTED;     // (model ensembles: inference only without the opt-in)
    if (!b->grad_ys || !b->adj || !b->workspace || !b->fwd.traj) return SNSDE_ERR_NULL;
    // increments: dW_out, or the supplied dW, or - MFMA Euler / Milstein adjoint, Philox with a host key - regenerated in-kernel
    if (!b->fwd.dW_out && !b->fwd.dW && b->fwd.seed_dev) return SNSDE_ERR_NULL;
    SnsdeNet net;
    rc = snsde_build_net(b->fwd.model, b->fwd.n_steps, &net);
    if (rc) return rc;
    const snsde_mfma::BackwardRoute r = route_backward(&b->fwd, net);
    if (r.mode == 0) return SNSDE_ERR_UNSUPPORTED;
    if (r.mode == 2) {
        if (!b->fwd.dW_out) return SNSDE_ERR_NULL;
        if (b->flags & SNSDE_BWD_ADJ0_ONLY) return SNSDE_ERR_OPTION;     // (its parameter pass reads every a_n)
        if (b->delta_save) return SNSDE_ERR_UNSUPPORTED;    // the generic adjoint writes adjoints only
        if (b->workspace_bytes < backward_workspace_bytes(b, net, r)) return SNSDE_ERR_WORKSPACE;
        return snsde_generic_backward_launch(b, net, static_cast<hipStream_t>(hip_stream));
    }
    if (!b->fwd.act_save) return SNSDE_ERR_NULL;
    if (b->workspace_bytes < backward_workspace_bytes(b, net, r)) return SNSDE_ERR_WORKSPACE;
    return snsde_mfma_backward_launch(b, net, r, static_cast<hipStream_t>(hip_stream), (int)step_offset);
}

size_t snsde_param_gradients_workspace_bytes(const snsde_backward* b) {
    if (!b || b->struct_size != sizeof(snsde_backward) || b->fwd.struct_size != sizeof(snsde_solve)) return 0;
    SnsdeNet net;
    if (snsde_build_net(b->fwd.model, b->fwd.n_steps, &net)) return 0;
    const snsde_mfma::BackwardRoute r = route_backward(&b->fwd, net);
    if (r.mode != 1) return 0;
    return snsde_wgrad_workspace_floats(b, net, r.members) * sizeof(float);
}

// The checks the two parameter-gradient entry points share once the descriptor's pointers are in: the route (MFMA adjoint only),
// the delta planes, the two workspaces
static int route_param_gradients(const snsde_backward* b, const SnsdeNet& net, size_t pg_workspace_bytes, snsde_mfma::BackwardRoute* r) {
    *r = route_backward(&b->fwd, net);
    if (r->mode != 1) return SNSDE_ERR_UNSUPPORTED;
    if (!b->delta_save && r->rp.kernel != snsde_mfma::RevKernel::w4_fused) return SNSDE_ERR_NULL;      // (delta_slots == 0: no planes)
    // the adjoint's workspace is an INPUT of the parameter pass (its per-workgroup diffusion-side sums; on the wave-group path the
    // per-tile weight-gradient blocks themselves): the descriptor must still carry it, at the size the adjoint was given
    if (!b->workspace) return SNSDE_ERR_NULL;
    if (b->workspace_bytes < backward_workspace_bytes(b, net, *r)) return SNSDE_ERR_WORKSPACE;
    if (pg_workspace_bytes < snsde_wgrad_workspace_floats(b, net, r->members) * sizeof(float)) return SNSDE_ERR_WORKSPACE;
    return SNSDE_OK;
}

int snsde_param_gradients(const snsde_backward* b, float* grad_params, void* workspace, size_t workspace_bytes,
                          void* hip_stream) {
    if (!b || !grad_params || !workspace) return SNSDE_ERR_NULL;
    if (b->struct_size != sizeof(snsde_backward)) return SNSDE_ERR_ABI;
    int rc = validate_solve(&b->fwd, false);
    if (rc) return rc;
    if (snsde_members(&b->fwd) > 1 && !ensemble_grad(&b->fwd)) return SNSDE_ERR_UNSUPPORTED;      // (model ensembles: inference only without the opt-in)
    if (!b->adj || !b->fwd.traj || !b->fwd.act_save || !b->fwd.workspace)
        return SNSDE_ERR_NULL;
    SnsdeNet net;
    rc = snsde_build_net(b->fwd.model, b->fwd.n_steps, &net);
    if (rc) return rc;
    snsde_mfma::BackwardRoute r;
    rc = route_param_gradients(b, net, workspace_bytes, &r);
    if (rc) return rc;
    return snsde_wgrad_launch(b, net, r, grad_params, (int32_t)snsde_param_numel(&b->fwd.model), static_cast<float*>(workspace),
                              static_cast<hipStream_t>(hip_stream));
}

int snsde_backward_with_gradients(const snsde_backward* b, float* grad_params, void* pg_workspace, size_t pg_workspace_bytes,
                                  void* hip_stream) {
    return snsde_backward_with_gradients_at(b, grad_params, pg_workspace, pg_workspace_bytes, 0, hip_stream);
}

int snsde_backward_with_gradients_at(const snsde_backward* b, float* grad_params, void* pg_workspace, size_t pg_workspace_bytes,
                                     int64_t step_offset, void* hip_stream) {
    if (!b || !grad_params || !pg_workspace) return SNSDE_ERR_NULL;
    if (b->struct_size != sizeof(snsde_backward)) return SNSDE_ERR_ABI;
    int rc = validate_solve(&b->fwd, false);
    if (rc) return rc;
    if ((rc = check_backward_offset(&b->fwd, step_offset)) != SNSDE_OK) return rc;
    if (snsde_members(&b->fwd) > 1 && !ensemble_grad(&b->fwd)) return SNSDE_ERR_UNSUPPORTED;      // (model ensembles: inference only without the opt-in)
    if (!b->grad_ys || !b->adj || !b->workspace || !b->fwd.traj || !b->fwd.act_save || !b->fwd.workspace)
        return SNSDE_ERR_NULL;
    if (!b->fwd.dW_out && !b->fwd.dW && b->fwd.seed_dev) return SNSDE_ERR_NULL;
    SnsdeNet net;
    rc = snsde_build_net(b->fwd.model, b->fwd.n_steps, &net);
    if (rc) return rc;
    snsde_mfma::BackwardRoute r;
    rc = route_param_gradients(b, net, pg_workspace_bytes, &r);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    rc = snsde_mfma_backward_launch(b, net, r, st, (int)step_offset);
    if (rc) return rc;
    return snsde_wgrad_launch(b, net, r, grad_params, (int32_t)snsde_param_numel(&b->fwd.model), static_cast<float*>(pg_workspace), st);
}

// The checks of snsde_coeff_gradients that need no pointer: the configurations it covers (mode 1 with delta planes, the reference's
// Diffusion_model fields, no accumulator column; sample paths where route_backward plans them).  *delta_slots: the planes per pass of delta_save
static int route_coeff_gradients(const snsde_solve* s, int32_t* delta_slots) {
    if (s->flags & SNSDE_FLAG_BF16_OPERANDS) return SNSDE_ERR_UNSUPPORTED;      // (also under SNSDE_FLAG_BF16_GRAD: M is not rounded here)
    if (s->kl_column1 != 0 || snsde_solve_variant(s)) return SNSDE_ERR_UNSUPPORTED;
    if (snsde_members(s) > 1) return SNSDE_ERR_UNSUPPORTED;      // (a sum over members of delta_p M_m, one M_m per member: not built)
    SnsdeNet net;
    int rc = snsde_build_net(s->model, s->n_steps, &net);
    if (rc) return rc;
    if (route_backward(s, net).mode != 1) return SNSDE_ERR_UNSUPPORTED;
    rc = snsde_save_layout(s, nullptr, nullptr, delta_slots);
    if (rc) return rc;
    return *delta_slots > 0 ? SNSDE_OK : SNSDE_ERR_UNSUPPORTED;      // (0: the wave-pair adjoint leaves no delta planes)
}

size_t snsde_coeff_gradients_workspace_bytes(const snsde_backward* b) {
    if (!b || b->struct_size != sizeof(snsde_backward) || b->fwd.struct_size != sizeof(snsde_solve)) return 0;
    if (validate_model(&b->fwd.model) || b->fwd.batch <= 0 || b->fwd.knots < 2 || b->fwd.n_steps <= 0) return 0;
    int32_t dslots = 0;
    if (route_coeff_gradients(&b->fwd, &dslots)) return 0;
    return snsde_cgrad_workspace_floats(b->fwd) * sizeof(float);
}

int snsde_coeff_gradients(const snsde_backward* b, float* grad_coeffs, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!b || !grad_coeffs || !workspace) return SNSDE_ERR_NULL;
    if (b->struct_size != sizeof(snsde_backward)) return SNSDE_ERR_ABI;
    int rc = validate_solve(&b->fwd, false);
    if (rc) return rc;
    int32_t dslots = 0;
    rc = route_coeff_gradients(&b->fwd, &dslots);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!snsde_cgrad_reads_x(b->fwd.model)) return snsde_cgrad_zero_launch(b->fwd, grad_coeffs, st);      // the drift does not read X: exactly zero
    if (!b->delta_save) return SNSDE_ERR_UNSUPPORTED;
    if (workspace_bytes < snsde_cgrad_workspace_floats(b->fwd) * sizeof(float)) return SNSDE_ERR_WORKSPACE;
    SnsdeNet net;
    rc = snsde_build_net(b->fwd.model, b->fwd.n_steps, &net);
    if (rc) return rc;
    return snsde_cgrad_launch(b, net, dslots, grad_coeffs, static_cast<float*>(workspace), st);
}

int snsde_spline_evaluate(const float* coeffs, int32_t batch, int32_t knots, int32_t channels, int32_t index,
                          float frac, int32_t derivative, float* out, void* hip_stream) {
    if (!coeffs || !out) return SNSDE_ERR_NULL;
    if (batch <= 0 || knots < 2 || channels <= 0) return SNSDE_ERR_DIMS;
    if (index < 0 || index > knots - 2) return SNSDE_ERR_INDEX;
    return snsde_spline_launch(coeffs, batch, knots, channels, index, frac, derivative, out,
                               static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
