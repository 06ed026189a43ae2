// encode_host.h — what dhw_encode / dhw_encode_workspace_bytes (include/dhw.h) decide without a device: the ranges, the
// workspace size and every argument rule.  Plain C++ (no HIP header), as page/page_host.h.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

constexpr int ENCODE_MAX_B = 65535;    // one workgroup per line on grid.x
constexpr int ENCODE_MIN_N = 2;
constexpr int ENCODE_MAX_N = 4096;     // points per line: the line stays in LDS as fp64 (encode.hip)
constexpr int ENCODE_MIN_L = 8;
constexpr int ENCODE_MAX_L = 4096;
constexpr int ENCODE_MAX_ROUNDS = 8;

// A line of ENCODE_MAX_N points fits in LDS (84 KiB of the CU's 160), so nothing is spilled and no workspace is needed at any
// admitted shape.  The argument stays in the ABI so that a later layout can spill without changing it.
inline size_t encode_workspace_bytes(int B, int N) {
  (void)B;
  (void)N;
  return 0;
}

// Every argument rule of dhw_encode: 0 on success, else -1 with the offending argument named in msg.  Pointers are only
// compared and never dereferenced.
inline int encode_check_args(const void* points, int B, int N, int L, int rounds, float max_abs, const void* strokes_out,
                             const void* lens_out, const void* status_out, const void* workspace, size_t workspace_bytes, char* msg,
                             size_t msg_len) {
  if (B < 1 || B > ENCODE_MAX_B) { snprintf(msg, msg_len, "B must be in [1, %d] (got %d)", ENCODE_MAX_B, B); return -1; }
  if (N < ENCODE_MIN_N || N > ENCODE_MAX_N) { snprintf(msg, msg_len, "N must be in [%d, %d] (got %d)", ENCODE_MIN_N, ENCODE_MAX_N, N); return -1; }
  if (L < ENCODE_MIN_L || L > ENCODE_MAX_L) { snprintf(msg, msg_len, "L must be in [%d, %d] (got %d)", ENCODE_MIN_L, ENCODE_MAX_L, L); return -1; }
  if (rounds < 0 || rounds > ENCODE_MAX_ROUNDS) { snprintf(msg, msg_len, "rounds must be in [0, %d] (got %d)", ENCODE_MAX_ROUNDS, rounds); return -1; }
  if (!std::isfinite(max_abs) || !(max_abs > 0.f)) { snprintf(msg, msg_len, "max_abs must be finite and > 0 (got %g)", (double)max_abs); return -1; }
  if (!points) { snprintf(msg, msg_len, "points is NULL"); return -1; }
  if (!strokes_out) { snprintf(msg, msg_len, "strokes_out is NULL"); return -1; }
  if (!lens_out) { snprintf(msg, msg_len, "lens_out is NULL"); return -1; }
  if (!status_out) { snprintf(msg, msg_len, "status_out is NULL"); return -1; }
  if (workspace_bytes < encode_workspace_bytes(B, N)) {
    snprintf(msg, msg_len, "workspace_bytes %zu < dhw_encode_workspace_bytes(%d, %d) = %zu", workspace_bytes, B, N, encode_workspace_bytes(B, N));
    return -1;
  }
  if (((uintptr_t)points | (uintptr_t)strokes_out | (uintptr_t)workspace) & 15) {
    snprintf(msg, msg_len, "points, strokes_out and workspace must be 16-byte aligned");
    return -1;
  }
  if (((uintptr_t)lens_out | (uintptr_t)status_out) & 3) { snprintf(msg, msg_len, "lens_out and status_out must be 4-byte aligned"); return -1; }
  return 0;
}
