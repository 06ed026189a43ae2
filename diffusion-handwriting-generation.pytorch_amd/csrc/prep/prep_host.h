// prep_host.h — what dhw_prep / dhw_prep_workspace_bytes (include/dhw.h) decide without a device: the ranges, the workspace
// size and every argument rule.  Plain C++ (no HIP header), as encode/encode_host.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

constexpr int PREP_MAX_B = 65535;      // one image per grid.z
constexpr int PREP_MAX_HIN = 4096;
constexpr int PREP_MIN_WIN = 16;
constexpr int PREP_MAX_WIN = 16384;    // a multiple of 16: the box pass loads 16 bytes per lane
constexpr int PREP_MIN_H = 8;
constexpr int PREP_MAX_H = 512;
constexpr int PREP_MIN_W = 8;
constexpr int PREP_MAX_W = 4096;       // a multiple of 4: the resize pass stores 16 bytes per thread

// the crop boxes, int32 [B][4] = (first row, last row, first column, last column) with a dark pixel
inline size_t prep_workspace_bytes(int B) { return (B < 1 || B > PREP_MAX_B) ? 0 : (size_t)B * 4 * sizeof(int32_t); }

// Every argument rule of dhw_prep: 0 on success, else -1 with the offending argument named in msg.  Pointers are only
// compared and never dereferenced.
inline int prep_check_args(const void* images, const void* sizes, int B, int Hin, int Win, int H, int W, int thresh, const void* img_out,
                           const void* widths_out, const void* boxes_out, const void* status_out, const void* workspace,
                           size_t workspace_bytes, char* msg, size_t msg_len) {
  if (B < 1 || B > PREP_MAX_B) { snprintf(msg, msg_len, "B must be in [1, %d] (got %d)", PREP_MAX_B, B); return -1; }
  if (Hin < 1 || Hin > PREP_MAX_HIN) { snprintf(msg, msg_len, "Hin must be in [1, %d] (got %d)", PREP_MAX_HIN, Hin); return -1; }
  if (Win < PREP_MIN_WIN || Win > PREP_MAX_WIN || Win % 16) {
    snprintf(msg, msg_len, "Win must be a multiple of 16 in [%d, %d] (got %d)", PREP_MIN_WIN, PREP_MAX_WIN, Win);
    return -1;
  }
  if (H < PREP_MIN_H || H > PREP_MAX_H) { snprintf(msg, msg_len, "H must be in [%d, %d] (got %d)", PREP_MIN_H, PREP_MAX_H, H); return -1; }
  if (W < PREP_MIN_W || W > PREP_MAX_W || W % 4) {
    snprintf(msg, msg_len, "W must be a multiple of 4 in [%d, %d] (got %d)", PREP_MIN_W, PREP_MAX_W, W);
    return -1;
  }
  if ((long long)B * H * W >= (1ll << 31)) { snprintf(msg, msg_len, "B H W must be < 2^31 (got %lld)", (long long)B * H * W); return -1; }
  if (thresh < 1 || thresh > 255) { snprintf(msg, msg_len, "thresh must be in [1, 255] (got %d)", thresh); return -1; }
  if (!images) { snprintf(msg, msg_len, "images is NULL"); return -1; }
  if (!img_out) { snprintf(msg, msg_len, "img_out is NULL"); return -1; }
  if (!status_out) { snprintf(msg, msg_len, "status_out is NULL"); return -1; }
  if (!workspace) { snprintf(msg, msg_len, "workspace is NULL"); return -1; }
  if (((uintptr_t)images | (uintptr_t)img_out | (uintptr_t)workspace) & 15) {
    snprintf(msg, msg_len, "images, img_out and workspace must be 16-byte aligned");
    return -1;
  }
  if (((uintptr_t)sizes | (uintptr_t)widths_out | (uintptr_t)boxes_out | (uintptr_t)status_out) & 3) {
    snprintf(msg, msg_len, "sizes, widths_out, boxes_out and status_out must be 4-byte aligned");
    return -1;
  }
  if (workspace_bytes < prep_workspace_bytes(B)) {
    snprintf(msg, msg_len, "workspace_bytes %zu < dhw_prep_workspace_bytes(%d) = %zu", workspace_bytes, B, prep_workspace_bytes(B));
    return -1;
  }
  return 0;
}
