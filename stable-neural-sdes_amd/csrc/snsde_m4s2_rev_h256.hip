// Two-tile adjoint of the H = 256 Euler / Milstein solve (snsde_m4s2_rev_kernel.h): instantiations and dispatch.
#include "snsde_m4s2_rev_kernel.h"

namespace snsde_mfma {

// (NHID, GEO): make_rev_plan names this kernel (RevKernel::two_tile_h256) where m4s2_rev_instantiated says so and sends everything
// else to the general kernel, streamed weights (same results)
#ifdef SNSDE_DEV_SUBSET
#define SNSDE_M4S2_REV_LIST(X) X(1, 0)
#else
#define SNSDE_M4S2_REV_LIST(X) X(0, 1) X(0, 0) X(1, 1) X(1, 0) X(2, 1) X(2, 0)
#endif

bool m4s2_rev_instantiated(int nhid, bool geo) {
#define SNSDE_R2(NH_, GEO_) if (nhid == NH_ && geo == (GEO_ != 0)) return true;
    SNSDE_M4S2_REV_LIST(SNSDE_R2)
#undef SNSDE_R2
    return false;
}

int dispatch_rev_h256_two_tile(const RevPlan& p, const RevArgs& a, hipStream_t st) {
    // what the kernel covers (make_rev_plan plans it for nothing else): the reference's own fields on 4-row tiles, elementwise
    // diffusions, y-dependent drifts, no path-integral column
    if (!p.FL || p.SRK || p.IO0 || p.NN != 0 || a.act_fn != 0 || a.f_out != 0 || a.g_out != 0 || a.acc_col >= 0) return SNSDE_ERR_UNSUPPORTED;
#define SNSDE_R2(NH_, GEO_) if (p.NHID == NH_ && (p.GEO != 0) == (GEO_ != 0)) return launch_rev2<CfgS2R<NH_, GEO_>>(a, st);
    SNSDE_M4S2_REV_LIST(SNSDE_R2)
#undef SNSDE_R2
    return SNSDE_ERR_UNSUPPORTED;
}

}  // namespace snsde_mfma
