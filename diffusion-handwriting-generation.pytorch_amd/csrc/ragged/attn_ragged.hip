// ragged/attn_ragged.hip — attn.hip compiled with per-sample lengths (AttnParams.lens; dhw_kernels.h, DHW_LENS): the stroke-side
// attention launches of ragged calls on the one-launch-per-GEMM path.  The uniform build in attn.hip is unchanged.
#define DHW_LENS 1
#define launch_attn launch_attn_ragged
#include "../attn.hip"
