// Lean 4-row-tile forward kernel with bf16 MFMA operands (snsde_m4b_kernel.h) instantiated for hidden size 128.
#include "snsde_m4b_kernel.h"

namespace snsde_mfma {

int dispatch_lean_bf16_h128(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) { return dispatch_lean_bf16<128>(p, a, st); }

}  // namespace snsde_mfma
