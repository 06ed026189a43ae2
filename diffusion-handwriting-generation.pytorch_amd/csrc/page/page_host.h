// page_host.h — what dhw_page / dhw_page_workspace_bytes (include/dhw.h) decide without a device: the workspace layout and
// every argument rule.  Plain C++ (tests/cpp/page_host_check.cpp compiles it alone).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

constexpr int PAGE_MAX_N = 4096;       // lines per call
constexpr int PAGE_MAX_L = 4096;       // one workgroup scans a line: 256 threads x 16 strokes (as the line rasteriser)
constexpr int PAGE_TILE_W = 32;        // columns per raster tile: 8 lanes x 4 pixels
constexpr int PAGE_BAND_H = 96;        // rows a workgroup keeps running minima for: 3 passes x 32 rows
constexpr int PAGE_THREADS = 256;
constexpr size_t PAGE_HEADER_BYTES = 32;    // sizeof(PageLineHeader), page.h
constexpr size_t PAGE_SEGMENT_BYTES = 16;   // one float4 per stroke

// workspace: [N] x PageLineHeader (32 bytes), then [N][L] x float4 segments
inline size_t page_workspace_bytes(int N, int L) {
  if (N < 1 || N > PAGE_MAX_N || L < 1 || L > PAGE_MAX_L) return 0;
  return (size_t)N * PAGE_HEADER_BYTES + (size_t)N * (size_t)L * PAGE_SEGMENT_BYTES;
}

// the geometry of a call, by value
struct PageGeometry {
  int P, H, W, lines_per_page;
  float margin_left, margin_top, pitch, line_width, scale;
};

// Every argument rule of dhw_page: 0 on success, else -1 with the offending argument named in msg.  Pointers are only
// compared and never dereferenced.
inline int page_check_args(const void* strokes, int N, int L, const PageGeometry& g, const void* pages, const void* scale_out,
                           const void* boxes_out, const void* workspace, size_t workspace_bytes, char* msg, size_t msg_len) {
  if (N < 1 || N > PAGE_MAX_N) { snprintf(msg, msg_len, "N must be in [1, %d] (got %d)", PAGE_MAX_N, N); return -1; }
  if (L < 1 || L > PAGE_MAX_L) { snprintf(msg, msg_len, "L must be in [1, %d] (got %d)", PAGE_MAX_L, L); return -1; }
  if (g.P < 1) { snprintf(msg, msg_len, "P must be >= 1 (got %d)", g.P); return -1; }
  if (g.H < 8) { snprintf(msg, msg_len, "H must be >= 8 (got %d)", g.H); return -1; }
  if (g.W < 8 || g.W % 4) { snprintf(msg, msg_len, "W must be >= 8 and a multiple of 4 (got %d)", g.W); return -1; }
  const long long rows = (long long)g.P * g.H;   // (below 2^62: the second product is formed only when it cannot overflow)
  if (rows >= (1LL << 31) || rows * g.W >= (1LL << 31)) {
    snprintf(msg, msg_len, "P x H x W must stay below 2^31 (P %d, H %d, W %d)", g.P, g.H, g.W);
    return -1;
  }
  const long long tiles = (g.W + PAGE_TILE_W - 1) / PAGE_TILE_W, bands = (g.H + PAGE_BAND_H - 1) / PAGE_BAND_H;
  if ((long long)g.P * tiles >= (1LL << 24) || bands > 65535) {
    snprintf(msg, msg_len, "P x W (or H) is beyond the launch grid (P %d, H %d, W %d)", g.P, g.H, g.W);
    return -1;
  }
  if (g.lines_per_page < 1) { snprintf(msg, msg_len, "lines_per_page must be >= 1 (got %d)", g.lines_per_page); return -1; }
  if (!std::isfinite(g.pitch) || !(g.pitch > 0.f)) { snprintf(msg, msg_len, "pitch must be finite and > 0 (got %g)", (double)g.pitch); return -1; }
  if (!std::isfinite(g.margin_left) || !(g.margin_left >= 0.f)) {
    snprintf(msg, msg_len, "margin_left must be finite and >= 0 (got %g)", (double)g.margin_left);
    return -1;
  }
  if (!std::isfinite(g.margin_top) || !(g.margin_top >= 0.f)) {
    snprintf(msg, msg_len, "margin_top must be finite and >= 0 (got %g)", (double)g.margin_top);
    return -1;
  }
  if (!((float)g.W - 2.f * g.margin_left > 0.f)) {
    snprintf(msg, msg_len, "margin_left %g leaves no room: W - 2 margin_left must be > 0 (W %d)", (double)g.margin_left, g.W);
    return -1;
  }
  if (!(g.line_width >= 0.5f && g.line_width <= 16.f)) { snprintf(msg, msg_len, "line_width must be in [0.5, 16] (got %g)", (double)g.line_width); return -1; }
  if (!std::isfinite(g.scale) || !(g.scale >= 0.f)) { snprintf(msg, msg_len, "scale must be finite and >= 0 (got %g)", (double)g.scale); return -1; }
  if (!strokes) { snprintf(msg, msg_len, "strokes is NULL"); return -1; }
  if (!pages) { snprintf(msg, msg_len, "pages is NULL"); return -1; }
  if (!scale_out) { snprintf(msg, msg_len, "scale_out is NULL"); return -1; }
  if (!boxes_out) { snprintf(msg, msg_len, "boxes_out is NULL"); return -1; }
  if (!workspace) { snprintf(msg, msg_len, "workspace is NULL"); return -1; }
  if (workspace_bytes < page_workspace_bytes(N, L)) {
    snprintf(msg, msg_len, "workspace_bytes %zu < dhw_page_workspace_bytes(%d, %d) = %zu", workspace_bytes, N, L, page_workspace_bytes(N, L));
    return -1;
  }
  if (((uintptr_t)workspace | (uintptr_t)pages) & 15) { snprintf(msg, msg_len, "workspace and pages must be 16-byte aligned"); return -1; }
  if (((uintptr_t)scale_out | (uintptr_t)boxes_out) & 3) { snprintf(msg, msg_len, "scale_out and boxes_out must be 4-byte aligned"); return -1; }
  return 0;
}
