// dhw_prep_api.cpp — C-ABI of the writer-image preparation (include/dhw.h: dhw_prep_workspace_bytes, dhw_prep): the argument
// rules of prep_host.h (all before the first HIP call, so they answer on a machine without a GPU) and the three launches of
// prep.hip.  No handle, no allocation, no synchronisation, no host read of sizes or boxes: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "prep.h"

extern "C" {

size_t dhw_prep_workspace_bytes(int B) { return prep_workspace_bytes(B); }

int dhw_prep(const uint8_t* images, const int32_t* sizes, int B, int Hin, int Win, int H, int W, int thresh, float* img_out,
             int32_t* widths_out, int32_t* boxes_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_prep", int, {
    char msg[200];
    if (prep_check_args(images, sizes, B, Hin, Win, H, W, thresh, img_out, widths_out, boxes_out, status_out, workspace, workspace_bytes, msg,
                        sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_prep: %s", msg);
    const hipError_t e = launch_prep(images, sizes, B, Hin, Win, H, W, thresh, img_out, widths_out, boxes_out, status_out, (int32_t*)workspace,
                                     (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_prep: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
