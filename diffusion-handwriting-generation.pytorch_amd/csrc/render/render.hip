// render.hip — the stroke rasteriser (include/dhw.h: dhw_render): sampled strokes [B,L,3] -> grey-level line
// images [B,1,H,W] in the layout dhw_style_forward consumes.  Two kernels:
//   render_prepare_kernel  one workgroup per row: prefix sum of the offsets, pen lifts, the box of the drawn ink, the scale,
//                          and the drawn segments in pixel coordinates, compacted in stroke order into the workspace
//   render_raster_kernel   one workgroup per (row, 32-column tile, 96-row band): cull the row's segments against the tile in
//                          LDS chunks, then an exact distance field: min over segments of the distance to each pixel centre
// The minimum is exact and commutative and nothing is accumulated with atomics, so the picture is bit-deterministic.
#include "line_raster.h"
#include "render.h"

namespace {

using LR = LineRaster<RENDER_THREADS, RENDER_ITEMS, RENDER_TILE_W, RENDER_BAND_H, RENDER_CHUNK>;

__global__ __launch_bounds__(RENDER_THREADS) void render_prepare_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                                        int L, int H, int W, float line_width,
                                                                        RenderRowHeader* __restrict__ hdr, float4* __restrict__ segs,
                                                                        int32_t* __restrict__ widths_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);   // (the API documents 1 <= n <= L; a bad device-side entry must not read out of bounds)

  LR::Scan sc;
  LR::scan(strokes + (size_t)b * L * 3, n, sc);
  const int total = sc.total;
  const float xmin = sc.xmin, xmax = sc.xmax, ymin = sc.ymin, ymax = sc.ymax;

  if (total == 0) {   // no lift, or nothing before the last one: a white image of width 0
    if (tid == 0) {
      hdr[b] = RenderRowHeader{0, 0};
      if (widths_out) widths_out[b] = 0;
    }
    return;
  }

  const float m = 0.5f * line_width + 1.f;
  const float availh = (float)H - 2.f * m, availw = (float)W - 2.f * m;
  const float extx = xmax - xmin, exty = ymax - ymin;
  float s;
  if (exty > 0.f) {
    s = availh / exty;
    if (extx * s > availw) s = availw / extx;
  } else if (extx > 0.f) {
    s = fminf(availw / extx, availh);
  } else {
    s = 1.f;
  }
  const float voff = 0.5f * (availh - exty * s);
  const float yb = m + voff;

  float4* out = segs + (size_t)b * L + sc.off;
#pragma unroll
  for (int j = 0; j < RENDER_ITEMS; ++j) {
    if ((sc.drawn >> j) & 1u)
      *out++ = make_float4(m + (sc.ax(j) - xmin) * s, yb + (ymax - sc.ay(j)) * s, m + (sc.px[j] - xmin) * s, yb + (ymax - sc.py[j]) * s);
  }
  if (tid == 0) {
    const int wd = min(W, max(0, (int)ceilf(extx * s + 2.f * m)));
    hdr[b] = RenderRowHeader{total, wd};
    if (widths_out) widths_out[b] = wd;
  }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_raster_kernel(const RenderRowHeader* __restrict__ hdr, const float4* __restrict__ segs,
                                                                       int tiles, int L, int H, int W, float line_width,
                                                                       float* __restrict__ img) {
  __shared__ LR::Chunk s_chunk;   // x relative to the tile origin, y absolute

  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int tid = threadIdx.x;
  const int x0 = tile * RENDER_TILE_W;
  const int lx = tid % LR::LANES_X;
  const int col = x0 + 4 * lx;
  const int row0 = blockIdx.z * RENDER_BAND_H + tid / LR::LANES_X;
  const RenderRowHeader h = hdr[b];
  float* out = img + (size_t)b * H * W;

  if (x0 >= h.width) {   // wholly at or beyond the ink (a row without ink has width 0): white
    LR::store_white(out, row0, col, H, W);
    return;
  }

  const float radius = 0.5f * line_width + 0.5f;
  const float tlo = (float)x0 - radius, thi = (float)(x0 + RENDER_TILE_W) + radius;
  const float4* rs = segs + (size_t)b * L;
  const float cx = (float)(4 * lx) + 0.5f;   // centre of this lane's first pixel, relative to the tile origin
  // passes of this band that hold a row below H (workgroup-uniform: a scalar branch): a 32-row image costs 1 pass, not 3
  const int npass = min(LR::PASSES, (H - (int)blockIdx.z * RENDER_BAND_H + LR::ROWS_PER_PASS - 1) / LR::ROWS_PER_PASS);

  float mn[LR::PASSES][4];
#pragma unroll
  for (int p = 0; p < LR::PASSES; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) mn[p][q] = 1.0e30f;

  // the running minima stay in registers across chunks: a tile that keeps more than one chunk of segments drops none
  for (int base = 0; base < h.count; base += RENDER_CHUNK) {
    const int j = base + tid;
    bool keep = false;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < h.count) {
      s = rs[j];
      keep = fminf(s.x, s.z) < thi && fmaxf(s.x, s.z) > tlo;
    }
    const float abx = s.z - s.x, aby = s.w - s.y;
    const int kept = LR::compact(s_chunk, keep, make_float4(s.x - (float)x0, s.y, abx, aby));
    LR::min_dist2(s_chunk, kept, cx, row0, npass, mn);
    __syncthreads();   // the next round overwrites the chunk
  }

  LR::store_coverage(out, row0, col, H, W, radius, mn);
}

}  // namespace

hipError_t launch_render_prepare(const float* strokes, const int32_t* lens, int B, int L, int H, int W, float line_width,
                                 RenderRowHeader* hdr, float4* segs, int32_t* widths_out, hipStream_t st) {
  hipLaunchKernelGGL(render_prepare_kernel, dim3(B), dim3(RENDER_THREADS), 0, st, strokes, lens, L, H, W, line_width, hdr, segs, widths_out);
  return hipGetLastError();
}

hipError_t launch_render_raster(const RenderRowHeader* hdr, const float4* segs, int B, int L, int H, int W, float line_width,
                                float* img_out, hipStream_t st) {
  const int tiles = (W + RENDER_TILE_W - 1) / RENDER_TILE_W, bands = (H + RENDER_BAND_H - 1) / RENDER_BAND_H;
  hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)B * (unsigned)tiles, 1, bands), dim3(RENDER_THREADS), 0, st, hdr, segs, tiles, L, H, W,
                     line_width, img_out);
  return hipGetLastError();
}
