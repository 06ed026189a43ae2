// dtw.h — dynamic time warping between two sets of stroke lines (include/dhw.h: dhw_dtw_workspace_bytes, dhw_dtw): the ranges,
// the columns a lane owns, the split of the queries over waves, the workspace and every argument rule, decided without a
// device, and the launcher of dtw.hip.  Shared by dtw.hip and dhw_dtw_api.cpp.  Definition of the results: include/dhw.h and
// DESIGN.md §39.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>

constexpr int DTW_MAX_N = 16384;               // lines per set
constexpr long long DTW_MAX_PAIRS = 1ll << 26; // M N
constexpr int DTW_MAX_L = 1024;                // rows per line: twice the model's longest line
constexpr int DTW_MAX_F = 4;                   // features per row
constexpr int DTW_LANES = 64;                  // one wave holds one reference line: lane l owns columns l C .. l C + C - 1
constexpr int DTW_THREADS = 256;               // four independent waves per workgroup (no LDS, no barrier)
constexpr int DTW_WAVES = DTW_THREADS / DTW_LANES;constexpr int DTW_FILL = 65536;                // waves the query split aims for: many times the 256 CUs x 4 SIMDs x up to 8 resident
                                               // ones, so that the last round of waves leaves little of the chip idle

inline bool dtw_dims_ok(int M, int N, int La, int Lb, int F) {
  return M >= 1 && M <= DTW_MAX_N && N >= 1 && N <= DTW_MAX_N && (long long)M * N <= DTW_MAX_PAIRS && La >= 1 && La <= DTW_MAX_L && Lb >= 1 &&
         Lb <= DTW_MAX_L && F >= 1 && F <= DTW_MAX_F;
}

// columns per lane: the smallest of 1, 2, 4, 8, 16 with 64 C >= Lb
inline int dtw_cols(int Lb) {
  int c = 1;
  while (c * DTW_LANES < Lb) c *= 2;
  return c;
}

// The M queries of one reference are cut into `splits` runs of consecutive queries, one wave each; a run is chained through
// the wave's pipeline, so its fill and drain are paid once.  Enough runs for DTW_FILL waves, never more than M.
inline int dtw_splits(int M, int N) {
  int s = (DTW_FILL + N - 1) / N;
  return s < 1 ? 1 : s > M ? M : s;
}

// The workspace: the [M,N] fp32 matrix the nearest pass reads when dist_out is NULL, rounded up to 16 bytes.  A function of
// (M, N) alone; La, Lb and F are arguments so that the layout can grow without a change of signature.
inline size_t dtw_workspace_bytes(int M, int N, int La, int Lb, int F) {
  return dtw_dims_ok(M, N, La, Lb, F) ? ((size_t)M * N * sizeof(float) + 15) / 16 * 16 : 0;
}

// ---------------------------------------------------------------- argument rules: 0, or -1 with the offending argument named in msg
#define DTW_FAIL(...) do { snprintf(msg, msg_len, __VA_ARGS__); return -1; } while (0)

// a pointer that must be given (or may be NULL when optional) and 16-byte aligned; never dereferenced
inline int dtw_check_ptr(const char* name, const void* p, bool optional, char* msg, size_t msg_len) {
  if (!p && !optional) DTW_FAIL("%s is NULL", name);
  if ((uintptr_t)p & 15) DTW_FAIL("%s must be 16-byte aligned", name);
  return 0;
}

inline int dtw_check(const void* a, const void* lens_a, int M, int La, const void* b, const void* lens_b, int N, int Lb, int F, int skip_diag,
                     const void* dist_out, const void* steps_out, const void* nearest_out, const void* nearest_idx, const void* ws, size_t ws_bytes,
                     char* msg, size_t msg_len) {
  if (M < 1 || M > DTW_MAX_N) DTW_FAIL("M must be in [1, %d] (got %d)", DTW_MAX_N, M);
  if (N < 1 || N > DTW_MAX_N) DTW_FAIL("N must be in [1, %d] (got %d)", DTW_MAX_N, N);
  if ((long long)M * N > DTW_MAX_PAIRS) DTW_FAIL("M N must be at most 2^26 (got M %d, N %d)", M, N);
  if (La < 1 || La > DTW_MAX_L) DTW_FAIL("La must be in [1, %d] (got %d)", DTW_MAX_L, La);
  if (Lb < 1 || Lb > DTW_MAX_L) DTW_FAIL("Lb must be in [1, %d] (got %d)", DTW_MAX_L, Lb);
  if (F < 1 || F > DTW_MAX_F) DTW_FAIL("F must be in [1, %d] (got %d)", DTW_MAX_F, F);
  if (skip_diag && M != N) DTW_FAIL("skip_diag needs M == N (got M %d, N %d)", M, N);
  if (!dist_out && !steps_out && !nearest_out) DTW_FAIL("dist_out, steps_out and nearest_out are all NULL: nothing to compute");
  if (nearest_idx && !nearest_out) DTW_FAIL("nearest_idx needs nearest_out (nearest_out is NULL)");
  if (dtw_check_ptr("a", a, false, msg, msg_len) || dtw_check_ptr("lens_a", lens_a, true, msg, msg_len) ||
      dtw_check_ptr("b", b, false, msg, msg_len) || dtw_check_ptr("lens_b", lens_b, true, msg, msg_len) ||
      dtw_check_ptr("dist_out", dist_out, true, msg, msg_len) || dtw_check_ptr("steps_out", steps_out, true, msg, msg_len) ||
      dtw_check_ptr("nearest_out", nearest_out, true, msg, msg_len) || dtw_check_ptr("nearest_idx", nearest_idx, true, msg, msg_len))
    return -1;
  const size_t need = dtw_workspace_bytes(M, N, La, Lb, F);
  if (ws_bytes < need) DTW_FAIL("ws_bytes %zu < dhw_dtw_workspace_bytes(%d, %d, %d, %d, %d) = %zu", ws_bytes, M, N, La, Lb, F, need);
  return dtw_check_ptr("ws", ws, false, msg, msg_len);
}

#undef DTW_FAIL

// ---------------------------------------------------------------- launcher (dtw.hip): no allocation, no synchronisation
struct DtwArgs {
  const float *a, *b;            // [M,La,F], [N,Lb,F]
  const int32_t *lens_a, *lens_b;   // [M], [N] or NULL
  int M, N, La, Lb, splits, normalize;
  float* dist;                   // [M,N]: dist_out, the workspace, or NULL when only steps are asked for
  int32_t* steps;                // [M,N] or NULL
};

hipError_t launch_dtw(const DtwArgs& p, int F, int skip_diag, float* nearest_out, int32_t* nearest_idx, hipStream_t st);
