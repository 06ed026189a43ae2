// ragged/convblock_ragged.hip — convblock.hip compiled with per-sample lengths (ConvBlockParams.lens; dhw_kernels.h, DHW_LENS): the
// fused ConvBlock launches of ragged calls.  The uniform build in convblock.hip keeps its instruction stream unchanged.
#define DHW_LENS 1
#define DHW_STORE_RT 1   // (the store policy is read at run time here: dhw_kernels.h)
#define launch_convblock launch_convblock_ragged
#define launch_convblock_chain launch_convblock_chain_ragged
#define convblock_chain_supported convblock_chain_supported_ragged
#define convblock_chain_auto convblock_chain_auto_ragged
#define convblock_init convblock_init_ragged
#include "../convblock.hip"
