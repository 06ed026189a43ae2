// page.hip — the page compositor (include/dhw.h: dhw_page): N sampled lines [N,L,3] -> P page images
// [P,1,H,W] at ONE scale shared by all lines, each line in its slot, overlapping ink composed by min.  Two kernels:
//   page_prepare_kernel  one workgroup per line: prefix sum of the offsets, pen lifts, the box of the drawn ink, the largest
//                        scale s_n at which the line fits its slot, and the drawn segments in stroke units relative to the
//                        box corner (xmin, ymax), compacted in stroke order into the workspace.  It needs no scale.
//   page_raster_kernel   one workgroup per (page, 32-column tile, 96-row band): s = min s_n over the headers, the lines of the
//                        page whose placed box meets the tile, then for those lines alone the cull of the line rasteriser
//                        (ballot + popcount into an LDS chunk) and an exact distance field over the segments of all of them
// min is exact and commutative and nothing is accumulated with atomics: the pages do not depend on the order of the lines.
// The scan of a line and the pieces of the raster are those of the line rasteriser: render/line_raster.h.
#include "../render/line_raster.h"
#include "page.h"

namespace {

using LR = LineRaster<PAGE_THREADS, PAGE_ITEMS, PAGE_TILE_W, PAGE_BAND_H, PAGE_CHUNK>;

__global__ __launch_bounds__(PAGE_THREADS) void page_prepare_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                                    const int32_t* __restrict__ slots, int L, long long nslots, float pitch,
                                                                    float availw, PageLineHeader* __restrict__ hdr, float4* __restrict__ segs) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);   // (the API documents 1 <= n <= L; a bad device-side entry must not read out of bounds)

  LR::Scan sc;
  LR::scan(strokes + (size_t)b * L * 3, n, sc);
  const int total = sc.total;
  const float xmin = sc.xmin, xmax = sc.xmax, ymin = sc.ymin, ymax = sc.ymax;

  const int slot = slots ? slots[b] : b;
  if (total == 0 || slot < 0 || (long long)slot >= nslots) {   // draws nothing and takes no part in the scale
    if (tid == 0) hdr[b] = PageLineHeader{0, 0.f, 0.f, 0.f, 0.f, __builtin_inff(), slot, 0};
    return;
  }

  const float ex = xmax - xmin, ey = ymax - ymin;
  float sn = __builtin_inff();
  if (ey > 0.f) sn = pitch / ey;                  // one fp32 division each: tests/page_ref.py repeats them bit for bit
  if (ex > 0.f) sn = fminf(sn, availw / ex);

  float4* out = segs + (size_t)b * L + sc.off;
#pragma unroll
  for (int j = 0; j < PAGE_ITEMS; ++j) {
    if ((sc.drawn >> j) & 1u)
      *out++ = make_float4(sc.ax(j) - xmin, ymax - sc.ay(j), sc.px[j] - xmin, ymax - sc.py[j]);   // y flipped: image rows go down
  }
  if (tid == 0) hdr[b] = PageLineHeader{total, xmin, ymax, ex, ey, sn, slot, 0};
}

// where a line's ink box lands on its page at scale s: (left, top, right, bottom) in page pixels
__device__ __forceinline__ float4 place_line(const PageLineHeader& h, float s, int lpp, float margin_left, float margin_top, float pitch) {
  const float top = margin_top + (float)(h.slot % lpp) * pitch;
  const float oy = top + (pitch - h.ey * s) * 0.5f;
  return make_float4(margin_left, oy, margin_left + h.ex * s, oy + h.ey * s);
}

__global__ __launch_bounds__(PAGE_THREADS) void page_raster_kernel(const PageLineHeader* __restrict__ hdr, const float4* __restrict__ segs, int N,
                                                                   int L, int tiles, int H, int W, int lpp, float margin_left,
                                                                   float margin_top, float pitch, float line_width, float scale,
                                                                   float* __restrict__ pages, float* __restrict__ scale_out,
                                                                   float* __restrict__ boxes_out) {
  __shared__ LR::Chunk s_chunk;          // relative to the origin of the tile and band
  __shared__ int s_line[PAGE_THREADS];   // the lines of one header round that reach this tile, in line order
  __shared__ int s_lcnt[LR::WAVES];

  const int p = blockIdx.x / tiles, tile = blockIdx.x - p * tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = tile * PAGE_TILE_W, y0 = blockIdx.z * PAGE_BAND_H;
  const int lx = tid % LR::LANES_X;
  const int col = x0 + 4 * lx;
  const int rloc = tid / LR::LANES_X;       // this lane's row in the first pass, relative to the band
  float* out = pages + (size_t)p * H * W;

  // the shared scale: the exact min of s_n over the lines that draw.  Every wave of every workgroup reads all headers (64 at
  // a time, no barrier) and gets the same bits, whatever the order.
  float s = scale;
  if (!(scale > 0.f)) {
    float m = __builtin_inff();
    for (int n = lane; n < N; n += 64)
      if (hdr[n].count > 0) m = fminf(m, hdr[n].s_n);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fminf(m, __shfl_xor(m, d));
    s = m < __builtin_inff() ? m : 1.f;
  }

  if (blockIdx.x == 0 && blockIdx.z == 0) {   // the designated workgroup reports the scale and where every line went
    for (int n = tid; n < N; n += PAGE_THREADS) {
      const PageLineHeader h = hdr[n];
      float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
      if (h.count > 0) box = place_line(h, s, lpp, margin_left, margin_top, pitch);
      boxes_out[4 * n] = box.x;
      boxes_out[4 * n + 1] = box.y;
      boxes_out[4 * n + 2] = box.z;
      boxes_out[4 * n + 3] = box.w;
    }
    if (tid == 0) *scale_out = s;
  }

  const float radius = 0.5f * line_width + 0.5f;
  const float tlo = (float)x0 - radius, thi = (float)(x0 + PAGE_TILE_W) + radius;
  const float blo = (float)y0 - radius, bhi = (float)(y0 + PAGE_BAND_H) + radius;
  // a line reaches this workgroup iff it draws, sits on this page, and its placed box widened by the radius meets the tile
  auto reaches = [&](int n) -> bool {
    if (n >= N) return false;
    const PageLineHeader h = hdr[n];
    if (h.count <= 0 || h.slot / lpp != p) return false;
    const float4 box = place_line(h, s, lpp, margin_left, margin_top, pitch);
    return box.x < thi && box.z > tlo && box.y < bhi && box.w > blo;
  };

  bool any = false;   // (per wave again, and the same in every wave: the white exit below needs no barrier)
  for (int nb = 0; nb < N && !any; nb += 64) any = __ballot(reaches(nb + lane)) != 0ull;
  if (!any) {
    LR::store_white(out, y0 + rloc, col, H, W);
    return;
  }

  const float cx = (float)(4 * lx) + 0.5f;   // centre of this lane's first pixel, relative to the tile origin
  // passes of this band that hold a row below H (workgroup-uniform: a scalar branch)
  const int npass = min(LR::PASSES, (H - y0 + LR::ROWS_PER_PASS - 1) / LR::ROWS_PER_PASS);

  float mn[LR::PASSES][4];
#pragma unroll
  for (int q = 0; q < LR::PASSES; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) mn[q][k] = 1.0e30f;

  for (int nb = 0; nb < N; nb += PAGE_THREADS) {
    // the lines of this round that reach the tile, compacted in line order
    const bool hit = reaches(nb + tid);
    const unsigned long long lvote = __ballot(hit);
    if (lane == 0) s_lcnt[wave] = __popcll(lvote);
    __syncthreads();
    int loff = __popcll(lvote & ((1ull << lane) - 1ull)), nhit = 0;
#pragma unroll
    for (int w = 0; w < LR::WAVES; ++w) {
      if (w < wave) loff += s_lcnt[w];
      nhit += s_lcnt[w];
    }
    if (hit) s_line[loff] = nb + tid;
    __syncthreads();

    for (int hl = 0; hl < nhit; ++hl) {
      const int ln = s_line[hl];               // every lane reads the same address
      const PageLineHeader h = hdr[ln];
      const float4 box = place_line(h, s, lpp, margin_left, margin_top, pitch);
      const float ox = box.x, oy = box.y;
      const float4* rs = segs + (size_t)ln * L;
      // the running minima stay in registers across chunks and across lines
      for (int base = 0; base < h.count; base += PAGE_CHUNK) {
        const int j = base + tid;
        bool keep = false;
        float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
        if (j < h.count) {
          const float4 r = rs[j];
          ax = ox + r.x * s;
          ay = oy + r.y * s;
          bx = ox + r.z * s;
          by = oy + r.w * s;
          keep = fminf(ax, bx) < thi && fmaxf(ax, bx) > tlo && fminf(ay, by) < bhi && fmaxf(ay, by) > blo;
        }
        const int kept = LR::compact(s_chunk, keep, make_float4(ax - (float)x0, ay - (float)y0, bx - ax, by - ay));
        LR::min_dist2(s_chunk, kept, cx, rloc, npass, mn);
        __syncthreads();   // the next round overwrites the chunk
      }
    }
    __syncthreads();   // the next header round overwrites the line list
  }

  LR::store_coverage(out, y0 + rloc, col, H, W, radius, mn);
}

}  // namespace

hipError_t launch_page_prepare(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, const PageGeometry& g,
                               PageLineHeader* hdr, float4* segs, hipStream_t st) {
  const long long nslots = (long long)g.P * g.lines_per_page;
  const float availw = (float)g.W - 2.f * g.margin_left;
  hipLaunchKernelGGL(page_prepare_kernel, dim3(N), dim3(PAGE_THREADS), 0, st, strokes, lens, slots, L, nslots, g.pitch, availw, hdr, segs);
  return hipGetLastError();
}

hipError_t launch_page_raster(const PageLineHeader* hdr, const float4* segs, int N, int L, const PageGeometry& g, float* pages,
                              float* scale_out, float* boxes_out, hipStream_t st) {
  const int tiles = (g.W + PAGE_TILE_W - 1) / PAGE_TILE_W, bands = (g.H + PAGE_BAND_H - 1) / PAGE_BAND_H;
  hipLaunchKernelGGL(page_raster_kernel, dim3((unsigned)g.P * (unsigned)tiles, 1, bands), dim3(PAGE_THREADS), 0, st, hdr, segs, N, L, tiles,
                     g.H, g.W, g.lines_per_page, g.margin_left, g.margin_top, g.pitch, g.line_width, g.scale, pages, scale_out, boxes_out);
  return hipGetLastError();
}
