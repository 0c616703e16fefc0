// Lean 4-row-tile forward kernel with bf16 MFMA operands (SNSDE_FLAG_BF16_OPERANDS): the instantiations of snsde_m4_kernel<CF>
// with CF = CfgBf16<CfgL<..>> (snsde_m4_kernel.h, "bf16 operands").  The reference's Diffusion_model fields (relu, elementwise
// diffusions), Euler / Milstein, H = 64 / 128; no path-integral column.  Inference (SAVE = 0, snsde_m4b_h*.hip) and, under
// SNSDE_FLAG_BF16_GRAD, training mode (SAVE = 1, snsde_m4bs_h*.hip: act_save / traj / dW_out hold the f32 values in front of the
// operand rounding; same states bit for bit).  make_plan decides (snsde_mfma.hip); a configuration outside this list has no plan,
// so the launch never reaches the refusals below.
#pragma once
#include "snsde_m4_kernel.h"

namespace snsde_mfma {

template <int H, int SAVE>
int dispatch_lean_bf16_cfg(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) {
    if (a.acc_col >= 0 || a.act != SNSDE_ACT_RELU || a.f_out != 0 || a.g_out != 0 || a.raw_time || a.gt_ext) return SNSDE_ERR_UNSUPPORTED;
#define SNSDE_LEANB(NH_, KX_, Y_) \
    if constexpr (lean_fits(H, NH_, KX_, Y_ != 0)) { \
        if (p.NHID == NH_ && p.KUXT == KX_ && (p.IO != 0) == (Y_ != 0)) return launch_lean<CfgBf16<CfgL<H, NH_, KX_, Y_, SAVE>>>(a, st); }
#define SNSDE_LEANBS(KX_, Y_) SNSDE_LEANB(0, KX_, Y_) SNSDE_LEANB(1, KX_, Y_) SNSDE_LEANB(2, KX_, Y_) SNSDE_LEANB(3, KX_, Y_)
#ifdef SNSDE_DEV_SUBSET
    SNSDE_LEANBS(1, 1) SNSDE_LEANBS(2, 1)
#else
    SNSDE_LEANBS(0, 1) SNSDE_LEANBS(1, 1) SNSDE_LEANBS(2, 1) SNSDE_LEANBS(3, 1) SNSDE_LEANBS(6, 1)
    SNSDE_LEANBS(1, 0) SNSDE_LEANBS(2, 0) SNSDE_LEANBS(3, 0) SNSDE_LEANBS(6, 0)
#endif
#undef SNSDE_LEANBS
#undef SNSDE_LEANB
    return SNSDE_ERR_UNSUPPORTED;
}

// training-mode instantiations, one translation unit per hidden size (snsde_m4bs_h*.hip)
int dispatch_lean_bf16_save_h64(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);
int dispatch_lean_bf16_save_h128(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st);

// inference; a launch with a save pointer set goes to the training-mode instantiations (make_plan lets it through under
// SNSDE_FLAG_BF16_GRAD only)
template <int H>
int dispatch_lean_bf16(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) {
    if (a.act_save || a.traj || a.dW_out) return H == 128 ? dispatch_lean_bf16_save_h128(p, a, st) : dispatch_lean_bf16_save_h64(p, a, st);
    return dispatch_lean_bf16_cfg<H, 0>(p, a, st);
}

}  // namespace snsde_mfma
