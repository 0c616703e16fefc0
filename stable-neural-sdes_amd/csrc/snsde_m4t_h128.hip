// Two-tiles-per-wave lean kernel (snsde_m4t_kernel.h) for hidden size 128: four waves, one per SIMD.  Instantiations and dispatch.
#include "snsde_m4t_kernel.h"

namespace snsde_mfma {

// (NHID, KUXT, training mode): make_plan takes this kernel under SNSDE_FLAG_TWO_TILE where it is instantiated
#define SNSDE_M4T_LIST(X) X(1, 2, 1) X(1, 1, 1)

bool m4t_instantiated(int nhid, int kuxt, bool save) {
#define SNSDE_LEAN2(NH_, KX_, TR_) if (nhid == NH_ && kuxt == KX_ && (TR_ || !save)) return true;
    SNSDE_M4T_LIST(SNSDE_LEAN2)
#undef SNSDE_LEAN2
    return false;
}

int dispatch_lean_h128_two_tile(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) {
    const bool save = a.act_save || a.traj || a.dW_out;
    if (p.IO == 0 || a.act != SNSDE_ACT_RELU || a.acc_col >= 0) return SNSDE_ERR_UNSUPPORTED;
#define SNSDE_LEAN2(NH_, KX_, TR_) \
    if (p.NHID == NH_ && p.KUXT == KX_ && (TR_ || !save)) \
        return save ? launch_lean2<CfgT<128, NH_, KX_, TR_>>(a, st) : launch_lean2<CfgT<128, NH_, KX_, 0>>(a, st);
    SNSDE_M4T_LIST(SNSDE_LEAN2)
#undef SNSDE_LEAN2
    return SNSDE_ERR_UNSUPPORTED;
}

}  // namespace snsde_mfma
