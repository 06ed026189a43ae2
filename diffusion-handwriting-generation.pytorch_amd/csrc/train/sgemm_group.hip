// sgemm_group.hip — sgemm_group_kernel (up to six GEMMs in one launch) per staging type.
#include "sgemm_core.h"

namespace dhw_train {

const SgGroupTable& sgemm_group_table() {
  static const SgGroupTable t = {{sgemm_group_kernel<float>, sgemm_group_kernel<bf16_t>}};
  return t;
}

}  // namespace dhw_train
