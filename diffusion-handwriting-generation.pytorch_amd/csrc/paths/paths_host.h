// paths_host.h — what dhw_paths / dhw_paths_workspace_bytes (include/dhw.h) decide without a device: the workspace layout and
// every argument rule.  Plain C++ (tests/cpp/paths_host_check.cpp compiles it alone).  The geometry rules are dhw_page's and
// are not repeated here: page_check_args (page/page_host.h) is asked, with stand-ins for what dhw_paths does not have.
#pragma once
#include "../page/page_host.h"

constexpr int PATHS_MAX_N = PAGE_MAX_N;     // lines per call
constexpr int PATHS_MAX_L = PAGE_MAX_L;     // one workgroup holds a line: 256 threads x 16 strokes (as the page compositor)
constexpr int PATHS_THREADS = PAGE_THREADS;
constexpr int PATHS_MAX_SMOOTH = 8;
constexpr int PATHS_MAX_ROUNDS = 8;

// workspace: [N] x float, the scale limit s_n of every line (+inf for a line that takes no part), padded to 16 bytes
inline size_t paths_workspace_bytes(int N, int L) {
  if (N < 1 || N > PATHS_MAX_N || L < 1 || L > PATHS_MAX_L) return 0;
  return ((size_t)N * sizeof(float) + 15) & ~(size_t)15;
}

// what dhw_paths adds to a page geometry, by value
struct PathsOptions {
  int smooth;
  float tol;
  int rounds;
};

// Every argument rule of dhw_paths: 0 on success, else -1 with the offending argument named in msg.  Pointers are only
// compared and never dereferenced; lens and slots may be NULL.  g.line_width is not an argument of dhw_paths and is ignored.
inline int paths_check_args(const void* strokes, const void* lens, const void* slots, int N, int L, const PageGeometry& g, const PathsOptions& o, const void* points_out,
                            const void* index_out, const void* counts_out, const void* scale_out, const void* boxes_out, const void* workspace,
                            size_t workspace_bytes, char* msg, size_t msg_len) {
  // N, L, the geometry and strokes: dhw_page's rules, asked with a valid line width, an aligned stand-in for the pointers
  // dhw_paths checks itself below, and a workspace that is never too small
  alignas(16) static const char stand_in[16] = {0};
  PageGeometry pg = g;
  pg.line_width = 2.f;
  if (page_check_args(strokes, N, L, pg, stand_in, stand_in, stand_in, stand_in, ~(size_t)0, msg, msg_len)) return -1;
  if (o.smooth < 0 || o.smooth > PATHS_MAX_SMOOTH) { snprintf(msg, msg_len, "smooth must be in [0, %d] (got %d)", PATHS_MAX_SMOOTH, o.smooth); return -1; }
  if (o.rounds < 0 || o.rounds > PATHS_MAX_ROUNDS) { snprintf(msg, msg_len, "rounds must be in [0, %d] (got %d)", PATHS_MAX_ROUNDS, o.rounds); return -1; }
  if (!std::isfinite(o.tol) || !(o.tol >= 0.f)) { snprintf(msg, msg_len, "tol must be finite and >= 0 (got %g)", (double)o.tol); return -1; }
  if (!points_out) { snprintf(msg, msg_len, "points_out is NULL"); return -1; }
  if (!index_out) { snprintf(msg, msg_len, "index_out is NULL"); return -1; }
  if (!counts_out) { snprintf(msg, msg_len, "counts_out is NULL"); return -1; }
  if (!scale_out) { snprintf(msg, msg_len, "scale_out is NULL"); return -1; }
  if (!boxes_out) { snprintf(msg, msg_len, "boxes_out is NULL"); return -1; }
  if (!workspace) { snprintf(msg, msg_len, "workspace is NULL"); return -1; }
  if (workspace_bytes < paths_workspace_bytes(N, L)) {
    snprintf(msg, msg_len, "workspace_bytes %zu < dhw_paths_workspace_bytes(%d, %d) = %zu", workspace_bytes, N, L, paths_workspace_bytes(N, L));
    return -1;
  }
  if (((uintptr_t)workspace | (uintptr_t)points_out) & 15) { snprintf(msg, msg_len, "workspace and points_out must be 16-byte aligned"); return -1; }
  if (((uintptr_t)strokes | (uintptr_t)lens | (uintptr_t)slots | (uintptr_t)index_out | (uintptr_t)counts_out | (uintptr_t)scale_out |
       (uintptr_t)boxes_out) & 3) {
    snprintf(msg, msg_len, "strokes, lens, slots, index_out, counts_out, scale_out and boxes_out must be 4-byte aligned");
    return -1;
  }
  return 0;
}
