// ragged/enclayer_ragged.hip — enclayer.hip compiled with per-sample lengths (EncLayerParams.lens; dhw_kernels.h, DHW_LENS): the
// fused EncoderLayer launches of ragged calls.  The uniform build in enclayer.hip keeps its instruction stream unchanged.
#define DHW_LENS 1
#define DHW_STORE_RT 1   // (the store policy is read at run time here: dhw_kernels.h)
#define launch_enclayer launch_enclayer_ragged
#define enclayer_supported enclayer_supported_ragged
#define enclayer_chain_supported enclayer_chain_supported_ragged
#define enclayer_init enclayer_init_ragged
#include "../enclayer.hip"
