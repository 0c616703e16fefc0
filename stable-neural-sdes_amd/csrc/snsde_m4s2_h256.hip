// H = 256 on 4-row tiles with a quarter of the weights resident (two tiles per wave): instantiations and dispatch.
// See snsde_m4s2_kernel.h.  relu fields only (the LipSwish / SiLU variants stay on snsde_m4s_kernel).
#include "snsde_m4s2_kernel.h"

namespace snsde_mfma {

// (NHID, KUXT, training mode): instantiated where the two tiles' working set + the resident blocks fit 256 registers without
// scratch (-Rpass-analysis=kernel-resource-usage, profiles/r06_h256_two_tile_resources.txt); make_plan sends everything else to
// the fully streamed kernel (same results)
#ifdef SNSDE_DEV_SUBSET
#define SNSDE_M4S2_LIST(X) X(1, 1, 1) X(1, 2, 0)
#else
#define SNSDE_M4S2_LIST(X) X(0, 0, 1) X(1, 0, 1) X(2, 0, 0) X(0, 1, 1) X(1, 1, 1) X(0, 2, 1) X(1, 2, 0)
#endif

bool m4s2_instantiated(int nhid, int kuxt, bool save) {
#define SNSDE_STREAM2(NH_, KX_, TR_) if (nhid == NH_ && kuxt == KX_ && (TR_ || !save)) return true;
    SNSDE_M4S2_LIST(SNSDE_STREAM2)
#undef SNSDE_STREAM2
    return false;
}

int dispatch_lean_h256_two_tile(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) {
    const bool save = a.act_save || a.traj || a.dW_out;
    if (p.IO == 0 || a.act != SNSDE_ACT_RELU) return SNSDE_ERR_UNSUPPORTED;
#define SNSDE_STREAM2(NH_, KX_, TR_) \
    if (p.NHID == NH_ && p.KUXT == KX_ && (TR_ || !save)) \
        return save ? launch_stream2<CfgS2<NH_, KX_, TR_>>(a, st) : launch_stream2<CfgS2<NH_, KX_, 0>>(a, st);
    SNSDE_M4S2_LIST(SNSDE_STREAM2)
#undef SNSDE_STREAM2
    return SNSDE_ERR_UNSUPPORTED;
}

}  // namespace snsde_mfma
