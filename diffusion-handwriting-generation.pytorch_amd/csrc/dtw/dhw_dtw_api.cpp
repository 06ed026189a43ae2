// dhw_dtw_api.cpp — C-ABI of the dynamic time warping between stroke lines (include/dhw.h: dhw_dtw_workspace_bytes, dhw_dtw): the
// argument rules of dtw.h (all before the first HIP call, so they answer on a machine without a GPU) and the launches of
// dtw.hip.  No handle, no allocation, no synchronisation: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "dtw.h"

extern "C" {

size_t dhw_dtw_workspace_bytes(int M, int N, int La, int Lb, int F) { return dtw_workspace_bytes(M, N, La, Lb, F); }

int dhw_dtw(const float* a, const int32_t* lens_a, int M, int La, const float* b, const int32_t* lens_b, int N, int Lb, int F, int normalize,
            int skip_diag, float* dist_out, int32_t* steps_out, float* nearest_out, int32_t* nearest_idx, void* ws, size_t ws_bytes,
            void* hip_stream) {
  GLOBAL_GUARD("dhw_dtw", int, {
    char msg[200];
    if (dtw_check(a, lens_a, M, La, b, lens_b, N, Lb, F, skip_diag, dist_out, steps_out, nearest_out, nearest_idx, ws, ws_bytes, msg, sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_dtw: %s", msg);
    DtwArgs p = {};
    p.a = a; p.b = b; p.lens_a = lens_a; p.lens_b = lens_b;
    p.M = M; p.N = N; p.La = La; p.Lb = Lb;
    p.splits = dtw_splits(M, N);
    p.normalize = normalize != 0;
    p.dist = dist_out ? dist_out : nearest_out ? (float*)ws : nullptr;   // the nearest pass reads the matrix: it lies in ws when not asked for
    p.steps = steps_out;
    const hipError_t e = launch_dtw(p, F, skip_diag, nearest_out, nearest_idx, (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_dtw: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
