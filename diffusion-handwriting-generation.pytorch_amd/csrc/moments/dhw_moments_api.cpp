// dhw_moments_api.cpp — C-ABI of the feature moments (include/dhw.h: dhw_moments_workspace_bytes, dhw_moments_update): the
// argument rules of moments.h (all before the first HIP call, so they answer on a machine without a GPU) and the launches of
// moments.hip.  No handle, no allocation, no synchronisation: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "moments.h"

extern "C" {

size_t dhw_moments_workspace_bytes(int N, int S, int D) { return moments_workspace_bytes(N, S, D); }

int dhw_moments_update(const float* feat, int N, int S, int D, double* sum, double* gram, void* ws, size_t ws_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_moments_update", int, {
    char msg[200];
    if (moments_check_args(feat, N, S, D, sum, gram, ws, ws_bytes, msg, sizeof msg)) return global_fail(DHW_ERR_ARG, "dhw_moments_update: %s", msg);
    const hipError_t e = launch_moments(feat, N, S, D, sum, gram, (double*)ws, (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_moments_update: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
