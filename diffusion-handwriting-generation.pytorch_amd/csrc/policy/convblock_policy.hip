// policy/convblock_policy.hip — convblock.hip compiled with the copy-outs' store policy read from ConvBlockParams.store /
// EncLayerParams.store_a at run time (dhw_kernels.h, DHW_STORE_RT): the fused ConvBlock launches of a handle created with a
// DHW_STORE_POLICY other than the default.  The build in convblock.hip has the default compiled in and carries no selection.
#define DHW_STORE_RT 1
#define launch_convblock launch_convblock_policy
#define launch_convblock_chain launch_convblock_chain_policy
#define convblock_chain_supported convblock_chain_supported_policy
#define convblock_chain_auto convblock_chain_auto_policy
#define convblock_init convblock_init_policy
#include "../convblock.hip"
