// dhw_truth_api.cpp — C-ABI of the page ground truth (include/dhw.h: dhw_truth_workspace_bytes, dhw_truth): the argument rules
// of truth_host.h (all before the first HIP call, so they answer on a machine without a GPU) and the launches of truth.hip:
// prepare, then place (left out when the caller gives the scale: prepare places the boxes itself), then the label map (left
// out when labels_out is NULL).  No handle, no allocation, no synchronisation: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "truth.h"

extern "C" {

size_t dhw_truth_workspace_bytes(int N, int L, int G) { return truth_workspace_bytes(N, L, G); }

int dhw_truth(const float* strokes, const int32_t* lens, const int32_t* slots, const int32_t* groups, int N, int L, int G, int P, int H, int W,
              int lines_per_page, float margin_left, float margin_top, float pitch, float line_width, float scale, float* boxes_out,
              int32_t* spans_out, int32_t* labels_out, float* scale_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_truth", int, {
    const PageGeometry g{P, H, W, lines_per_page, margin_left, margin_top, pitch, line_width, scale};
    char msg[200];
    if (truth_check_args(strokes, lens, slots, groups, N, L, G, g, boxes_out, spans_out, labels_out, scale_out, workspace, workspace_bytes, msg,
                         sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_truth: %s", msg);

    hipStream_t st = (hipStream_t)hip_stream;
    const TruthWorkspace w = truth_workspace(workspace, N, L);
    hipError_t e = launch_truth_prepare(strokes, lens, slots, groups, N, L, G, g, labels_out != nullptr, w, boxes_out, spans_out, scale_out, st);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_truth: prepare launch: %s", hipGetErrorString(e));
    if (!(scale > 0.f)) {
      e = launch_truth_place(N, G, g, w, boxes_out, spans_out, scale_out, st);
      if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_truth: place launch: %s", hipGetErrorString(e));
    }
    if (labels_out) {
      e = launch_truth_labels(N, L, g, w, labels_out, st);
      if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_truth: labels launch: %s", hipGetErrorString(e));
    }
    return 0;
  });
}

}  // extern "C"
