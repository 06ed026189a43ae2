// dhw_page_api.cpp — C-ABI of the page compositor (include/dhw.h: dhw_page_workspace_bytes, dhw_page): the argument rules of
// page_host.h (all before the first HIP call, so they answer on a machine without a GPU) and the two launches of page.hip.
// No handle, no allocation, no synchronisation: the call can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../../include/dhw.h"
#include "../host/error.h"
#include "page.h"

extern "C" {

size_t dhw_page_workspace_bytes(int N, int L) { return page_workspace_bytes(N, L); }

int dhw_page(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, int P, int H, int W, int lines_per_page,
             float margin_left, float margin_top, float pitch, float line_width, float scale, float* pages, float* scale_out,
             float* boxes_out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  GLOBAL_GUARD("dhw_page", int, {
    const PageGeometry g{P, H, W, lines_per_page, margin_left, margin_top, pitch, line_width, scale};
    char msg[200];
    if (page_check_args(strokes, N, L, g, pages, scale_out, boxes_out, workspace, workspace_bytes, msg, sizeof msg))
      return global_fail(DHW_ERR_ARG, "dhw_page: %s", msg);

    hipStream_t st = (hipStream_t)hip_stream;
    PageLineHeader* hdr = (PageLineHeader*)workspace;
    float4* segs = (float4*)((char*)workspace + (size_t)N * PAGE_HEADER_BYTES);
    hipError_t e = launch_page_prepare(strokes, lens, slots, N, L, g, hdr, segs, st);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_page: prepare launch: %s", hipGetErrorString(e));
    e = launch_page_raster(hdr, segs, N, L, g, pages, scale_out, boxes_out, st);
    if (e != hipSuccess) return global_fail(DHW_ERR_HIP, "dhw_page: raster launch: %s", hipGetErrorString(e));
    return 0;
  });
}

}  // extern "C"
