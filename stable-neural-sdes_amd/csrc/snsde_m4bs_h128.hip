// Lean 4-row-tile forward kernel with bf16 MFMA operands in training mode (snsde_m4b_kernel.h, SNSDE_FLAG_BF16_GRAD) instantiated
// for hidden size 128.
#include "snsde_m4b_kernel.h"

namespace snsde_mfma {

int dispatch_lean_bf16_save_h128(const MfmaPlan& p, const MfmaArgs& a, hipStream_t st) { return dispatch_lean_bf16_cfg<128, 1>(p, a, st); }

}  // namespace snsde_mfma
