// sgemm_bf16.hip — sgemm_tiled_kernel with bf16 staging (mixed-precision training): the 32 load-form / Conv1d variants.
#include "sgemm_core.h"

namespace dhw_train {

const SgBf16Table& sgemm_bf16_table() {
  static const SgBf16Table t = {{DHW_SG16(bf16_t, false), DHW_SG16(bf16_t, true)}};
  return t;
}

}  // namespace dhw_train
