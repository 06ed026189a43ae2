// dhw_render_api.cpp — C-ABI of the stroke rasteriser (include/dhw.h: dhw_render_workspace_bytes, dhw_render): argument
// checks (all before the first HIP call, so they answer on a machine without a GPU) and the two launches of render.hip.
// No handle, no allocation, no synchronisation: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "render.h"

extern "C" {

size_t dhw_render_workspace_bytes(int B, int L) {
  if (B < 1 || L < 1 || L > RENDER_MAX_L) return 0;
  return render_workspace_bytes(B, L);
}

int dhw_render(const float* strokes, const int32_t* lens, int B, int L, int H, int W, float line_width, float* img_out,
               int32_t* widths_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_render", int, {
    if (B < 1) return global_fail(DHW_ERR_ARG, "dhw_render: B must be >= 1 (got %d)", B);
    if (L < 1 || L > RENDER_MAX_L) return global_fail(DHW_ERR_ARG, "dhw_render: L must be in [1, %d] (got %d)", RENDER_MAX_L, L);
    if (H < 8) return global_fail(DHW_ERR_ARG, "dhw_render: H must be >= 8 (got %d)", H);
    if (W < 8 || W % 4) return global_fail(DHW_ERR_ARG, "dhw_render: W must be >= 8 and a multiple of 4 (got %d)", W);
    if (!(line_width >= 0.5f && line_width <= 16.f)) return global_fail(DHW_ERR_ARG, "dhw_render: line_width must be in [0.5, 16] (got %g)", (double)line_width);
    const float m2 = line_width + 2.f;   // 2 m: the margin on both sides
    if (!(m2 < (float)H && m2 < (float)W))
      return global_fail(DHW_ERR_ARG, "dhw_render: line_width %g needs line_width + 2 < H and < W (H %d, W %d)", (double)line_width, H, W);
    if (!strokes) return global_fail(DHW_ERR_ARG, "dhw_render: strokes is NULL");
    if (!img_out) return global_fail(DHW_ERR_ARG, "dhw_render: img_out is NULL");
    if (!workspace) return global_fail(DHW_ERR_ARG, "dhw_render: workspace is NULL");
    if (workspace_bytes < render_workspace_bytes(B, L))
      return global_fail(DHW_ERR_ARG, "dhw_render: workspace_bytes %zu < dhw_render_workspace_bytes(%d, %d) = %zu", workspace_bytes, B, L,
                         render_workspace_bytes(B, L));
    if (((uintptr_t)workspace | (uintptr_t)img_out) & 15)
      return global_fail(DHW_ERR_ARG, "dhw_render: workspace and img_out must be 16-byte aligned");
    const long long tiles = (W + RENDER_TILE_W - 1) / RENDER_TILE_W, bands = (H + RENDER_BAND_H - 1) / RENDER_BAND_H;
    if ((long long)B * tiles > INT_MAX || bands > 65535)
      return global_fail(DHW_ERR_ARG, "dhw_render: B x W (or H) is beyond the launch grid (B %d, H %d, W %d)", B, H, W);

    hipStream_t st = (hipStream_t)hip_stream;
    RenderRowHeader* hdr = (RenderRowHeader*)workspace;
    float4* segs = (float4*)((char*)workspace + render_header_bytes(B));
    hipError_t e = launch_render_prepare(strokes, lens, B, L, H, W, line_width, hdr, segs, widths_out, st);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_render: prepare launch: %s", hipGetErrorString(e));
    e = launch_render_raster(hdr, segs, B, L, H, W, line_width, img_out, st);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_render: raster launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
