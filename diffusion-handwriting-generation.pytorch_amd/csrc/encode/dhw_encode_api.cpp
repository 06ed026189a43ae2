// dhw_encode_api.cpp — C-ABI of the stroke encoder (include/dhw.h: dhw_encode_workspace_bytes, dhw_encode): the argument rules
// of encode_host.h (all before the first HIP call, so they answer on a machine without a GPU) and the one launch of
// encode.hip.  No handle, no allocation, no synchronisation, no host read of counts: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "encode.h"

extern "C" {

size_t dhw_encode_workspace_bytes(int B, int N) { return encode_workspace_bytes(B, N); }

int dhw_encode(const float* points, const int32_t* counts, int B, int N, int L, int rounds, float max_abs, float* strokes_out,
               int32_t* lens_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_encode", int, {
    char msg[200];
    if (encode_check_args(points, B, N, L, rounds, max_abs, strokes_out, lens_out, status_out, workspace, workspace_bytes, msg, sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_encode: %s", msg);
    if ((uintptr_t)counts & 3) return global_fail(DHW_ERR_ARG, "dhw_encode: counts must be 4-byte aligned");
    const hipError_t e = launch_encode(points, counts, B, N, L, rounds, max_abs, strokes_out, lens_out, status_out, (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_encode: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
