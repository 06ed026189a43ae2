// dhw_pairs_api.cpp — C-ABI of the pairwise statistics (include/dhw.h: dhw_pairs_pool, dhw_pairs_workspace_bytes, dhw_pairs_knn,
// dhw_pairs_cover, dhw_pairs_polysum): the argument rules of pairs.h (all before the first HIP call, so they answer on a machine
// without a GPU) and the launches of pairs.hip.  No handle, no allocation, no synchronisation: the calls can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "pairs.h"

// DHW_PAIRS_SPLIT=<n>: the number of column splits (0 or unset: automatic), read at each call
static int forced_splits() {
  const char* e = getenv("DHW_PAIRS_SPLIT");
  return e ? atoi(e) : 0;
}

extern "C" {

int dhw_pairs_pool(const float* feat, int N, int S, int D, double* out, void* hip_stream) {
  GLOBAL_GUARD("dhw_pairs_pool", int, {
    char msg[200];
    if (pairs_check_pool(feat, N, S, D, out, msg, sizeof msg)) return global_fail(DHW_ERR_ARG, "dhw_pairs_pool: %s", msg);
    const hipError_t e = launch_moments_pool(feat, N, S, D, out, (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_pairs_pool: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

size_t dhw_pairs_workspace_bytes(int M, int N, int D) { return pairs_workspace_bytes(M, N, D); }

int dhw_pairs_knn(const double* x, int N, int D, int k, double* radius2, void* ws, size_t ws_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_pairs_knn", int, {
    char msg[200];
    if (pairs_check_knn(x, N, D, k, radius2, ws, ws_bytes, msg, sizeof msg)) return global_fail(DHW_ERR_ARG, "dhw_pairs_knn: %s", msg);
    const hipError_t e = launch_pairs_knn(x, N, D, k, radius2, (double*)ws, pairs_splits(N, N, forced_splits()), (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_pairs_knn: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

int dhw_pairs_cover(const double* q, int M, const double* ref, int N, int D, const double* radius2, int32_t* count, double* nearest2,
                    int32_t* nearest_idx, void* ws, size_t ws_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_pairs_cover", int, {
    char msg[200];
    if (pairs_check_cover(q, M, ref, N, D, radius2, count, nearest2, nearest_idx, ws, ws_bytes, msg, sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_pairs_cover: %s", msg);
    const hipError_t e = launch_pairs_cover(q, M, ref, N, D, radius2, count, nearest2, nearest_idx, (double*)ws, pairs_splits(M, N, forced_splits()),
                                            (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_pairs_cover: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

int dhw_pairs_polysum(const double* x, int M, const double* y, int N, int D, int skip_diag, double* out, void* ws, size_t ws_bytes,
                      void* hip_stream) {
  GLOBAL_GUARD("dhw_pairs_polysum", int, {
    char msg[200];
    if (pairs_check_polysum(x, M, y, N, D, skip_diag, out, ws, ws_bytes, msg, sizeof msg)) return global_fail(DHW_ERR_ARG, "dhw_pairs_polysum: %s", msg);
    const hipError_t e = launch_pairs_polysum(x, M, y, N, D, skip_diag, out, (double*)ws, pairs_splits(M, N, forced_splits()), (hipStream_t)hip_stream);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_pairs_polysum: launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
