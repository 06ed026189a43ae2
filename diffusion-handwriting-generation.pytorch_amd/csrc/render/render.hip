// render.hip — the stroke rasteriser (include/dhw.h: dhw_render): sampled strokes [B,L,3] -> grey-level line
// images [B,1,H,W] in the layout dhw_style_forward consumes.  Two kernels:
//   render_prepare_kernel  one workgroup per row: prefix sum of the offsets, pen lifts, the box of the drawn ink, the scale,
//                          and the drawn segments in pixel coordinates, compacted in stroke order into the workspace
//   render_raster_kernel   one workgroup per (row, 32-column tile, 96-row band): cull the row's segments against the tile in
//                          LDS chunks, then an exact distance field: min over segments of the distance to each pixel centre
// The minimum is exact and commutative and nothing is accumulated with atomics, so the picture is bit-deterministic.
#include "render.h"

namespace {

constexpr int LDS_STRIDE = RENDER_ITEMS * 3 + 1;   // 49 floats per thread: odd, so the per-thread reads are conflict-free
constexpr int WAVES = RENDER_THREADS / 64;

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

__global__ __launch_bounds__(RENDER_THREADS) void render_prepare_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                                        int L, int H, int W, float line_width,
                                                                        RenderRowHeader* __restrict__ hdr, float4* __restrict__ segs,
                                                                        int32_t* __restrict__ widths_out) {
  __shared__ float s_in[RENDER_THREADS * LDS_STRIDE];
  __shared__ float s_sum[WAVES][2];
  __shared__ int s_last[WAVES];
  __shared__ float s_box[WAVES][4];
  __shared__ int s_cnt[WAVES];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);   // (the API documents 1 <= n <= L; a bad device-side entry must not read out of bounds)

  // rows at or past n are never read
  const float* src = strokes + (size_t)b * L * 3;
  for (int k = tid; k < 3 * n; k += RENDER_THREADS) {
    const int i = k / 3, c = k - 3 * i;
    s_in[(i / RENDER_ITEMS) * LDS_STRIDE + (i % RENDER_ITEMS) * 3 + c] = src[k];
  }
  __syncthreads();

  // thread t owns strokes [16 t, 16 t + 16): the summation order is a function of the stroke index, not of L or n
  const int i0 = tid * RENDER_ITEMS;
  float* mine = s_in + tid * LDS_STRIDE;
  float px[RENDER_ITEMS], py[RENDER_ITEMS];
  unsigned lift = 0;
  int last = -1;
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int j = 0; j < RENDER_ITEMS; ++j) {
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
  for (int j = 0; j < RENDER_ITEMS; ++j) {
    px[j] += basex;
    py[j] += basey;
  }
  mine[0] = px[RENDER_ITEMS - 1];
  mine[1] = py[RENDER_ITEMS - 1];
  __syncthreads();
  const float prevx = tid ? mine[-LDS_STRIDE] : 0.f, prevy = tid ? mine[1 - LDS_STRIDE] : 0.f;

  // segment i = pos[i-1] -> pos[i] is drawn iff 1 <= i < last and row i is not a lift
  unsigned drawn = 0;
  float xmin = 3.0e38f, xmax = -3.0e38f, ymin = 3.0e38f, ymax = -3.0e38f;
#pragma unroll
  for (int j = 0; j < RENDER_ITEMS; ++j) {
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

  float4* out = segs + (size_t)b * L + off;
#pragma unroll
  for (int j = 0; j < RENDER_ITEMS; ++j) {
    if ((drawn >> j) & 1u) {
      const float ax = j ? px[j - 1] : prevx, ay = j ? py[j - 1] : prevy;
      *out++ = make_float4(m + (ax - xmin) * s, yb + (ymax - ay) * s, m + (px[j] - xmin) * s, yb + (ymax - py[j]) * s);
    }
  }
  if (tid == 0) {
    const int wd = min(W, max(0, (int)ceilf(extx * s + 2.f * m)));
    hdr[b] = RenderRowHeader{total, wd};
    if (widths_out) widths_out[b] = wd;
  }
}

constexpr int LANES_X = RENDER_TILE_W / 4;                 // 8 lanes across a tile row, four adjacent pixels each
constexpr int ROWS_PER_PASS = RENDER_THREADS / LANES_X;    // 32
constexpr int PASSES = RENDER_BAND_H / ROWS_PER_PASS;      // 3
static_assert(RENDER_CHUNK == RENDER_THREADS, "one cull round of the workgroup fills at most one chunk");

__global__ __launch_bounds__(RENDER_THREADS) void render_raster_kernel(const RenderRowHeader* __restrict__ hdr, const float4* __restrict__ segs,
                                                                       int tiles, int L, int H, int W, float line_width,
                                                                       float* __restrict__ img) {
  __shared__ float4 s_seg[RENDER_CHUNK];   // (ax, ay, bx - ax, by - ay), x relative to the tile origin
  __shared__ float s_inv[RENDER_CHUNK];    // 1 / |b - a|^2, 0 for a zero-length segment (a point)
  __shared__ int s_cnt[WAVES];

  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = tile * RENDER_TILE_W;
  const int lx = tid % LANES_X;
  const int col = x0 + 4 * lx;
  const int row0 = blockIdx.z * RENDER_BAND_H + tid / LANES_X;
  const RenderRowHeader h = hdr[b];
  float* out = img + (size_t)b * H * W;

  if (x0 >= h.width) {   // wholly at or beyond the ink (a row without ink has width 0): white
    if (col < W) {
      const float4 white = make_float4(255.f, 255.f, 255.f, 255.f);
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int r = row0 + p * ROWS_PER_PASS;
        if (r < H) *reinterpret_cast<float4*>(out + (size_t)r * W + col) = white;
      }
    }
    return;
  }

  const float radius = 0.5f * line_width + 0.5f;
  const float tlo = (float)x0 - radius, thi = (float)(x0 + RENDER_TILE_W) + radius;
  const float4* rs = segs + (size_t)b * L;
  const float cx = (float)(4 * lx) + 0.5f;   // centre of this lane's first pixel, relative to the tile origin
  // passes of this band that hold a row below H (workgroup-uniform: a scalar branch): a 32-row image costs 1 pass, not 3
  const int npass = min(PASSES, (H - (int)blockIdx.z * RENDER_BAND_H + ROWS_PER_PASS - 1) / ROWS_PER_PASS);

  float mn[PASSES][4];
#pragma unroll
  for (int p = 0; p < PASSES; ++p)
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
      const float abx = s.z - s.x, aby = s.w - s.y;
      const float len2 = abx * abx + aby * aby;
      s_seg[off] = make_float4(s.x - (float)x0, s.y, abx, aby);
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
      for (int p = 0; p < PASSES; ++p) {
        if (p >= npass) break;
        const float dy = (float)(row0 + p * ROWS_PER_PASS) + 0.5f - a.y;
        const float dyab = dy * a.w;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float t = fminf(fmaxf((dxab[q] + dyab) * inv, 0.f), 1.f);
          const float ex = dx[q] - t * a.z, ey = dy - t * a.w;
          mn[p][q] = fminf(mn[p][q], ex * ex + ey * ey);
        }
      }
    }
    __syncthreads();   // the next round overwrites the chunk
  }

  if (col < W) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = row0 + p * ROWS_PER_PASS;
      if (r < H) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float cov = fminf(fmaxf(radius - sqrtf(mn[p][q]), 0.f), 1.f);
          v[q] = 255.f * (1.f - cov);
        }
        *reinterpret_cast<float4*>(out + (size_t)r * W + col) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
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
