// sgemm_f32.hip — the kernels with fp32 staging (the exact-f32 MFMA) that take one or two GEMMs: sgemm_tiled_kernel in its 32 load-form /
// Conv1d variants and its eight 32-row-tile variants, and the eight sgemm_pair_kernel variants (weight gradient + data gradient).  The
// pair kernels stay in the unit of the tiled kernels whose sgemm_body specialisations they share: hipcc's inlining of the body's
// lambdas depends on how many kernels of a unit call them, and apart they compile to other code.
#include "sgemm_core.h"

namespace dhw_train {

const SgF32Table& sgemm_f32_table() {
#define DHW_SG32(AM_, BK_) sgemm_tiled_kernel<AM_, BK_, true, true, float, false, 32>, sgemm_tiled_kernel<AM_, BK_, true, true, float, true, 32>
#define DHW_SGP(CVA_, CVB_, GMB_) sgemm_pair_kernel<SgV<true, false, CVA_, 64>, SgV<false, false, CVB_, GMB_>>
  static const SgF32Table t = {{DHW_SG16(float, false), DHW_SG16(float, true)},
                               {DHW_SG32(false, false), DHW_SG32(false, true), DHW_SG32(true, false), DHW_SG32(true, true)},
                               {DHW_SGP(false, false, 64), DHW_SGP(false, false, 32), DHW_SGP(false, true, 64), DHW_SGP(false, true, 32),
                                DHW_SGP(true, false, 64),  DHW_SGP(true, false, 32),  DHW_SGP(true, true, 64),  DHW_SGP(true, true, 32)}};
#undef DHW_SGP
#undef DHW_SG32
  return t;
}

}  // namespace dhw_train
