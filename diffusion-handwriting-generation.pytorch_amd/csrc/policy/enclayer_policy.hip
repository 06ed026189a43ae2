// policy/enclayer_policy.hip — enclayer.hip compiled with the copy-outs' store policy read from EncLayerParams.store_a / store_bc
// at run time (dhw_kernels.h, DHW_STORE_RT): the fused EncoderLayer launches of a handle created with a DHW_STORE_POLICY other
// than the default.  The build in enclayer.hip has the default compiled in and carries no selection.
#define DHW_STORE_RT 1
#define launch_enclayer launch_enclayer_policy
#define enclayer_supported enclayer_supported_policy
#define enclayer_chain_supported enclayer_chain_supported_policy
#define enclayer_init enclayer_init_policy
#include "../enclayer.hip"
