// render.h — launchers and layout of the stroke rasteriser (include/dhw.h: dhw_render); shared by render.hip and
// dhw_render_api.cpp.  Definition of the picture: include/dhw.h and DESIGN.md §17.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

constexpr int RENDER_MAX_L = 4096;     // one workgroup scans a row: 256 threads x 16 strokes
constexpr int RENDER_THREADS = 256;
constexpr int RENDER_ITEMS = RENDER_MAX_L / RENDER_THREADS;   // strokes per thread of the prepare kernel (fixed, so the
                                                              // summation order depends on the stroke index alone)
constexpr int RENDER_TILE_W = 32;      // columns per raster tile: 8 lanes x 4 pixels (32 beat 64)
constexpr int RENDER_BAND_H = 96;      // rows a workgroup keeps running minima for in registers: 3 passes x 32 rows
constexpr int RENDER_CHUNK = 256;      // segments per LDS chunk of the raster kernel (mirrored by vis.RENDER_CHUNK)

// workspace: [B] x {int count, int width} (padded to 16 bytes), then [B][L] x float4 (x0, y0, x1, y1) in pixel coordinates
struct RenderRowHeader { int32_t count, width; };
inline size_t render_header_bytes(int B) { return ((size_t)B * sizeof(RenderRowHeader) + 15) / 16 * 16; }
inline size_t render_workspace_bytes(int B, int L) { return render_header_bytes(B) + (size_t)B * (size_t)L * sizeof(float4); }

hipError_t launch_render_prepare(const float* strokes, const int32_t* lens, int B, int L, int H, int W, float line_width,
                                 RenderRowHeader* hdr, float4* segs, int32_t* widths_out, hipStream_t st);
hipError_t launch_render_raster(const RenderRowHeader* hdr, const float4* segs, int B, int L, int H, int W, float line_width,
                                float* img_out, hipStream_t st);
