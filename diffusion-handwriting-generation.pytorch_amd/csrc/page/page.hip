// page.hip — the page compositor (include/dhw.h: dhw_page): N sampled lines [N,L,3] -> P page images
// [P,1,H,W] at ONE scale shared by all lines, each line in its slot, overlapping ink composed by min.  Two kernels:
//   page_prepare_kernel  one workgroup per line: prefix sum of the offsets, pen lifts, the box of the drawn ink, the largest
//                        scale s_n at which the line fits its slot, and the drawn segments in stroke units relative to the
//                        box corner (xmin, ymax), compacted in stroke order into the workspace.  It needs no scale.
//   page_raster_kernel   one workgroup per (page, 32-column tile, 96-row band): s = min s_n over the headers, the lines of the
//                        page whose placed box meets the tile, then for those lines alone the cull of the line rasteriser
//                        (ballot + popcount into an LDS chunk) and an exact distance field over the segments of all of them
// min is exact and commutative and nothing is accumulated with atomics: the pages do not depend on the order of the lines.
// The scan of the prepare kernel is the one of render/render.hip written again (that file keeps it in an anonymous namespace
// and is not edited here; DESIGN.md §24 lists the shared header as a later refactor).
#include "page.h"

namespace {

constexpr int LDS_STRIDE = PAGE_ITEMS * 3 + 1;   // 49 floats per thread: odd, so the per-thread reads are conflict-free
constexpr int WAVES = PAGE_THREADS / 64;

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(PAGE_THREADS) void page_prepare_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                                    const int32_t* __restrict__ slots, int L, long long nslots, float pitch,
                                                                    float availw, PageLineHeader* __restrict__ hdr, float4* __restrict__ segs) {
  __shared__ float s_in[PAGE_THREADS * LDS_STRIDE];
  __shared__ float s_sum[WAVES][2];
  __shared__ int s_last[WAVES];
  __shared__ float s_box[WAVES][4];
  __shared__ int s_cnt[WAVES];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);   // (the API documents 1 <= n <= L; a bad device-side entry must not read out of bounds)

  // rows at or past n are never read
  const float* src = strokes + (size_t)b * L * 3;
  for (int k = tid; k < 3 * n; k += PAGE_THREADS) {
    const int i = k / 3, c = k - 3 * i;
    s_in[(i / PAGE_ITEMS) * LDS_STRIDE + (i % PAGE_ITEMS) * 3 + c] = src[k];
  }
  __syncthreads();

  // thread t owns strokes [16 t, 16 t + 16): the summation order is a function of the stroke index, not of L, n or N
  const int i0 = tid * PAGE_ITEMS;
  float* mine = s_in + tid * LDS_STRIDE;
  float px[PAGE_ITEMS], py[PAGE_ITEMS];
  unsigned lift = 0;
  int last = -1;
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int j = 0; j < PAGE_ITEMS; ++j) {
    if (i0 + j < n) {
      sx += mine[j * 3];
      sy += mine[j * 3 + 1];
      if (rintf(mine[j * 3 + 2]) != 0.f) {   // round-half-to-even, as np.round: 0.5 is not a lift
        lift |= 1u << j;
        last = i0 + j;
      }
    }
    px[j] = sx;
    py[j] = sy;
  }
  const float incx = wave_incl_scan(sx, lane), incy = wave_incl_scan(sy, lane);
  float basex = __shfl_up(incx, 1), basey = __shfl_up(incy, 1);
  if (lane == 0) basex = basey = 0.f;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d));
  if (lane == 63) {
    s_sum[wave][0] = incx;
    s_sum[wave][1] = incy;
  }
  if (lane == 0) s_last[wave] = last;
  __syncthreads();
  for (int w = 0; w < wave; ++w) {
    basex += s_sum[w][0];
    basey += s_sum[w][1];
  }
  last = s_last[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) last = max(last, s_last[w]);

  // positions; each thread leaves its last one in LDS so that segment 16 t starts exactly where segment 16 t - 1 ended
#pragma unroll
  for (int j = 0; j < PAGE_ITEMS; ++j) {
    px[j] += basex;
    py[j] += basey;
  }
  mine[0] = px[PAGE_ITEMS - 1];
  mine[1] = py[PAGE_ITEMS - 1];
  __syncthreads();
  const float prevx = tid ? mine[-LDS_STRIDE] : 0.f, prevy = tid ? mine[1 - LDS_STRIDE] : 0.f;

  // segment i = pos[i-1] -> pos[i] is drawn iff 1 <= i < last and row i is not a lift
  unsigned drawn = 0;
  float xmin = 3.0e38f, xmax = -3.0e38f, ymin = 3.0e38f, ymax = -3.0e38f;
#pragma unroll
  for (int j = 0; j < PAGE_ITEMS; ++j) {
    const int i = i0 + j;
    if (i >= 1 && i < last && !((lift >> j) & 1u)) {
      drawn |= 1u << j;
      const float ax = j ? px[j - 1] : prevx, ay = j ? py[j - 1] : prevy;
      xmin = fminf(xmin, fminf(ax, px[j]));
      xmax = fmaxf(xmax, fmaxf(ax, px[j]));
      ymin = fminf(ymin, fminf(ay, py[j]));
      ymax = fmaxf(ymax, fmaxf(ay, py[j]));
    }
  }
  const int mycnt = __popc(drawn);
  const int inccnt = wave_incl_scan(mycnt, lane);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    xmin = fminf(xmin, __shfl_xor(xmin, d));
    xmax = fmaxf(xmax, __shfl_xor(xmax, d));
    ymin = fminf(ymin, __shfl_xor(ymin, d));
    ymax = fmaxf(ymax, __shfl_xor(ymax, d));
  }
  if (lane == 63) s_cnt[wave] = inccnt;
  if (lane == 0) {
    s_box[wave][0] = xmin;
    s_box[wave][1] = xmax;
    s_box[wave][2] = ymin;
    s_box[wave][3] = ymax;
  }
  __syncthreads();
  int off = inccnt - mycnt, total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) off += s_cnt[w];
    total += s_cnt[w];
    xmin = fminf(xmin, s_box[w][0]);
    xmax = fmaxf(xmax, s_box[w][1]);
    ymin = fminf(ymin, s_box[w][2]);
    ymax = fmaxf(ymax, s_box[w][3]);
  }

  const int slot = slots ? slots[b] : b;
  if (total == 0 || slot < 0 || (long long)slot >= nslots) {   // draws nothing and takes no part in the scale
    if (tid == 0) hdr[b] = PageLineHeader{0, 0.f, 0.f, 0.f, 0.f, __builtin_inff(), slot, 0};
    return;
  }

  const float ex = xmax - xmin, ey = ymax - ymin;
  float sn = __builtin_inff();
  if (ey > 0.f) sn = pitch / ey;                  // one fp32 division each: tests/page_ref.py repeats them bit for bit
  if (ex > 0.f) sn = fminf(sn, availw / ex);

  float4* out = segs + (size_t)b * L + off;
#pragma unroll
  for (int j = 0; j < PAGE_ITEMS; ++j) {
    if ((drawn >> j) & 1u) {
      const float ax = j ? px[j - 1] : prevx, ay = j ? py[j - 1] : prevy;
      *out++ = make_float4(ax - xmin, ymax - ay, px[j] - xmin, ymax - py[j]);   // y flipped: image rows go down
    }
  }
  if (tid == 0) hdr[b] = PageLineHeader{total, xmin, ymax, ex, ey, sn, slot, 0};
}

constexpr int LANES_X = PAGE_TILE_W / 4;                 // 8 lanes across a tile row, four adjacent pixels each
constexpr int ROWS_PER_PASS = PAGE_THREADS / LANES_X;    // 32
constexpr int PASSES = PAGE_BAND_H / ROWS_PER_PASS;      // 3
static_assert(PAGE_CHUNK == PAGE_THREADS, "one cull round of the workgroup fills at most one chunk");

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
  __shared__ float4 s_seg[PAGE_CHUNK];   // (ax, ay, bx - ax, by - ay) relative to the origin of the tile and band
  __shared__ float s_inv[PAGE_CHUNK];    // 1 / |b - a|^2, 0 for a zero-length segment (a point)
  __shared__ int s_cnt[WAVES];
  __shared__ int s_line[PAGE_THREADS];   // the lines of one header round that reach this tile, in line order
  __shared__ int s_lcnt[WAVES];

  const int p = blockIdx.x / tiles, tile = blockIdx.x - p * tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = tile * PAGE_TILE_W, y0 = blockIdx.z * PAGE_BAND_H;
  const int lx = tid % LANES_X;
  const int col = x0 + 4 * lx;
  const int rloc = tid / LANES_X;        // this lane's row in the first pass, relative to the band
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
    if (col < W) {
      const float4 white = make_float4(255.f, 255.f, 255.f, 255.f);
#pragma unroll
      for (int q = 0; q < PASSES; ++q) {
        const int r = y0 + rloc + q * ROWS_PER_PASS;
        if (r < H) *reinterpret_cast<float4*>(out + (size_t)r * W + col) = white;
      }
    }
    return;
  }

  const float cx = (float)(4 * lx) + 0.5f;   // centre of this lane's first pixel, relative to the tile origin
  // passes of this band that hold a row below H (workgroup-uniform: a scalar branch)
  const int npass = min(PASSES, (H - y0 + ROWS_PER_PASS - 1) / ROWS_PER_PASS);

  float mn[PASSES][4];
#pragma unroll
  for (int q = 0; q < PASSES; ++q)
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
    for (int w = 0; w < WAVES; ++w) {
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
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(vote);
        __syncthreads();
        int off = __popcll(vote & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
          if (w < wave) off += s_cnt[w];
          kept += s_cnt[w];
        }
        if (keep) {
          const float abx = bx - ax, aby = by - ay;
          const float len2 = abx * abx + aby * aby;
          s_seg[off] = make_float4(ax - (float)x0, ay - (float)y0, abx, aby);
          s_inv[off] = len2 > 0.f ? 1.f / len2 : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < kept; ++k) {
          const float4 a = s_seg[k];   // every lane reads the same address: an LDS broadcast
          const float inv = s_inv[k];
          float dx[4], dxab[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            dx[q] = cx + (float)q - a.x;
            dxab[q] = dx[q] * a.z;
          }
#pragma unroll
          for (int q = 0; q < PASSES; ++q) {
            if (q >= npass) break;
            const float dy = (float)(rloc + q * ROWS_PER_PASS) + 0.5f - a.y;
            const float dyab = dy * a.w;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float t = fminf(fmaxf((dxab[c] + dyab) * inv, 0.f), 1.f);
              const float ex = dx[c] - t * a.z, ey = dy - t * a.w;
              mn[q][c] = fminf(mn[q][c], ex * ex + ey * ey);
            }
          }
        }
        __syncthreads();   // the next round overwrites the chunk
      }
    }
    __syncthreads();   // the next header round overwrites the line list
  }

  if (col < W) {
#pragma unroll
    for (int q = 0; q < PASSES; ++q) {
      const int r = y0 + rloc + q * ROWS_PER_PASS;
      if (r < H) {
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float cov = fminf(fmaxf(radius - sqrtf(mn[q][c]), 0.f), 1.f);
          v[c] = 255.f * (1.f - cov);
        }
        *reinterpret_cast<float4*>(out + (size_t)r * W + col) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
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
