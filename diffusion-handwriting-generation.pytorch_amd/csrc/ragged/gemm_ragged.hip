// ragged/gemm_ragged.hip — gemm.hip compiled with per-sample lengths (GemmParams.lens; dhw_kernels.h, DHW_LENS): the launchers of the
// stroke-path GEMMs of ragged calls.  The uniform build in gemm.hip keeps its instruction stream unchanged.
#define DHW_LENS 1
#define launch_gemm launch_gemm_ragged
#define gemm_tile_for gemm_tile_for_ragged
#define gemm_init gemm_init_ragged
#include "../gemm.hip"
