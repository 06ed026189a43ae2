// dhw_paths_api.cpp — C-ABI of the vector twin of the page compositor (include/dhw.h: dhw_paths_workspace_bytes, dhw_paths):
// the argument rules of paths_host.h (all before the first HIP call, so they answer on a machine without a GPU) and the two
// launches of paths.hip; the first, which finds every line's scale limit, is left out when the caller gives the scale.
// No handle, no allocation, no synchronisation: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "paths.h"

extern "C" {

size_t dhw_paths_workspace_bytes(int N, int L) { return paths_workspace_bytes(N, L); }

int dhw_paths(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, int P, int H, int W, int lines_per_page,
              float margin_left, float margin_top, float pitch, float scale, int smooth, float tol, int rounds, float* points_out,
              int32_t* index_out, int32_t* counts_out, float* scale_out, float* boxes_out, void* workspace, size_t workspace_bytes,
              void* hip_stream) {
  GLOBAL_GUARD("dhw_paths", int, {
    const PageGeometry g{P, H, W, lines_per_page, margin_left, margin_top, pitch, 0.f, scale};
    const PathsOptions o{smooth, tol, rounds};
    char msg[200];
    if (paths_check_args(strokes, lens, slots, N, L, g, o, points_out, index_out, counts_out, scale_out, boxes_out, workspace, workspace_bytes, msg,
                         sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_paths: %s", msg);

    hipStream_t st = (hipStream_t)hip_stream;
    float* sn = (float*)workspace;
    if (!(scale > 0.f)) {
      const hipError_t e = launch_paths_limits(strokes, lens, slots, N, L, g, sn, st);
      if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_paths: limits launch: %s", hipGetErrorString(e));
    }
    const PathsOut out{(float4*)points_out, index_out, counts_out, scale_out, boxes_out};
    const hipError_t e = launch_paths(strokes, lens, slots, N, L, g, o, sn, out, st);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_paths: paths launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
