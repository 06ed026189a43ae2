// truth_host.h — what dhw_truth / dhw_truth_workspace_bytes (include/dhw.h) decide without a device: the workspace layout and
// every argument rule.  Plain C++ (tests/cpp/truth_host_check.cpp compiles it alone).  The geometry rules are dhw_page's and
// are not repeated here: page_check_args (page/page_host.h) is asked, with stand-ins for what dhw_truth does not have.
#pragma once
#include "../page/page_host.h"

constexpr int TRUTH_MAX_N = PAGE_MAX_N;     // lines per call
constexpr int TRUTH_MAX_L = PAGE_MAX_L;     // one workgroup holds a line: 256 threads x 16 strokes (as the page compositor)
constexpr int TRUTH_THREADS = PAGE_THREADS;
constexpr int TRUTH_MAX_G = 256;            // groups per line: the group table shares the 64 KB of LDS with the scan's 50 KB,
                                            // and one thread places one group
constexpr size_t TRUTH_ID_BYTES = 4;        // one int32 id per stroke

// workspace: [N] x PageLineHeader (32 bytes), [N][L] x float4 segments, [N][L] x int32 ids, padded to 16 bytes.  G changes
// nothing but the range check.
inline size_t truth_workspace_bytes(int N, int L, int G) {
  if (N < 1 || N > TRUTH_MAX_N || L < 1 || L > TRUTH_MAX_L || G < 1 || G > TRUTH_MAX_G) return 0;
  const size_t bytes = (size_t)N * PAGE_HEADER_BYTES + (size_t)N * (size_t)L * (PAGE_SEGMENT_BYTES + TRUTH_ID_BYTES);
  return (bytes + 15) & ~(size_t)15;
}

// Every argument rule of dhw_truth: 0 on success, else -1 with the offending argument named in msg.  Pointers are only
// compared and never dereferenced; lens, slots and labels_out may be NULL.
inline int truth_check_args(const void* strokes, const void* lens, const void* slots, const void* groups, int N, int L, int G, const PageGeometry& g,
                            const void* boxes_out, const void* spans_out, const void* labels_out, const void* scale_out, const void* workspace,
                            size_t workspace_bytes, char* msg, size_t msg_len) {
  // N, L, the geometry and strokes: dhw_page's rules, asked with an aligned stand-in for the pointers dhw_truth checks itself
  // below and a workspace that is never too small
  alignas(16) static const char stand_in[16] = {0};
  if (page_check_args(strokes, N, L, g, stand_in, stand_in, stand_in, stand_in, ~(size_t)0, msg, msg_len)) return -1;
  if (G < 1 || G > TRUTH_MAX_G) { snprintf(msg, msg_len, "G must be in [1, %d] (got %d)", TRUTH_MAX_G, G); return -1; }
  if (!groups) { snprintf(msg, msg_len, "groups is NULL"); return -1; }
  if (!boxes_out) { snprintf(msg, msg_len, "boxes_out is NULL"); return -1; }
  if (!spans_out) { snprintf(msg, msg_len, "spans_out is NULL"); return -1; }
  if (!scale_out) { snprintf(msg, msg_len, "scale_out is NULL"); return -1; }
  if (!workspace) { snprintf(msg, msg_len, "workspace is NULL"); return -1; }
  if (workspace_bytes < truth_workspace_bytes(N, L, G)) {
    snprintf(msg, msg_len, "workspace_bytes %zu < dhw_truth_workspace_bytes(%d, %d, %d) = %zu", workspace_bytes, N, L, G,
             truth_workspace_bytes(N, L, G));
    return -1;
  }
  if (((uintptr_t)workspace | (uintptr_t)labels_out) & 15) { snprintf(msg, msg_len, "workspace and labels_out must be 16-byte aligned"); return -1; }
  if (((uintptr_t)strokes | (uintptr_t)lens | (uintptr_t)slots | (uintptr_t)groups | (uintptr_t)boxes_out | (uintptr_t)spans_out |
       (uintptr_t)scale_out) & 3) {
    snprintf(msg, msg_len, "strokes, lens, slots, groups, boxes_out, spans_out and scale_out must be 4-byte aligned");
    return -1;
  }
  return 0;
}
