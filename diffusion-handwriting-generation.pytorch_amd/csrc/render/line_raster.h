// line_raster.h — what the line rasteriser (render.hip) and the page compositor (page/page.hip) do alike: the scan of one
// line's strokes in a workgroup, and the pieces of the exact distance-field raster of a (32-column tile, 96-row band).  Both
// promise bit-determinism and "a line in a batch has the bits of the line alone"; that rests on the summation order of this
// scan, so it is written once.  Each translation unit instantiates LineRaster with its own constants (render.h, page.h) and
// keeps what differs: where the segments go, the headers, the cull rule, the row convention.
#pragma once
#include <hip/hip_runtime.h>

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

template <int THREADS, int ITEMS, int TILE_W, int BAND_H, int CHUNK>
struct LineRaster {
  static constexpr int LDS_STRIDE = ITEMS * 3 + 1;   // 49 floats per thread: odd, so the per-thread reads are conflict-free
  static constexpr int WAVES = THREADS / 64;
  static constexpr int LANES_X = TILE_W / 4;                 // 8 lanes across a tile row, four adjacent pixels each
  static constexpr int ROWS_PER_PASS = THREADS / LANES_X;    // 32
  static constexpr int PASSES = BAND_H / ROWS_PER_PASS;      // 3
  static_assert(CHUNK == THREADS, "one cull round of the workgroup fills at most one chunk");

  // What the scan leaves in each thread.  Thread t owns strokes [ITEMS t, ITEMS t + ITEMS); segment i = pos[i-1] -> pos[i].
  struct Scan {
    float px[ITEMS], py[ITEMS];      // the positions after this thread's strokes
    float prevx, prevy;              // the position before them: exactly where thread t - 1 ended
    unsigned drawn;                  // bit j: segment ITEMS t + j is drawn
    int off, total;                  // drawn segments of the threads before this one, and of the line
    float xmin, xmax, ymin, ymax;    // the box of the drawn ink (the same in every thread)
    // where drawn segment j of this thread starts
    __device__ __forceinline__ float ax(int j) const { return j ? px[j - 1] : prevx; }
    __device__ __forceinline__ float ay(int j) const { return j ? py[j - 1] : prevy; }
  };

  // The scan of one line by the whole workgroup: src = its strokes [n][3], n already clamped to [0, ITEMS * THREADS].
  static __device__ __forceinline__ void scan(const float* src, int n, Scan& r) {
    __shared__ float s_in[THREADS * LDS_STRIDE];
    __shared__ float s_sum[WAVES][2];
    __shared__ int s_last[WAVES];
    __shared__ float s_box[WAVES][4];
    __shared__ int s_cnt[WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // rows at or past n are never read
    for (int k = tid; k < 3 * n; k += THREADS) {
      const int i = k / 3, c = k - 3 * i;
      s_in[(i / ITEMS) * LDS_STRIDE + (i % ITEMS) * 3 + c] = src[k];
    }
    __syncthreads();

    // the summation order is a function of the stroke index, not of L, n or the number of lines
    const int i0 = tid * ITEMS;
    float* mine = s_in + tid * LDS_STRIDE;
    float px[ITEMS], py[ITEMS];   // (locals, handed to r at the end: through r the compiler allocates other registers)
    unsigned lift = 0;
    int last = -1;
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
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
    for (int j = 0; j < ITEMS; ++j) {
      px[j] += basex;
      py[j] += basey;
    }
    mine[0] = px[ITEMS - 1];
    mine[1] = py[ITEMS - 1];
    __syncthreads();
    const float prevx = tid ? mine[-LDS_STRIDE] : 0.f;
    const float prevy = tid ? mine[1 - LDS_STRIDE] : 0.f;

    // segment i is drawn iff 1 <= i < last and row i is not a lift
    unsigned drawn = 0;
    float xmin = 3.0e38f, xmax = -3.0e38f, ymin = 3.0e38f, ymax = -3.0e38f;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
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
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      r.px[j] = px[j];
      r.py[j] = py[j];
    }
    r.prevx = prevx;
    r.prevy = prevy;
    r.drawn = drawn;
    r.off = off;
    r.total = total;
    r.xmin = xmin;
    r.xmax = xmax;
    r.ymin = ymin;
    r.ymax = ymax;
  }

  // One chunk of culled segments in LDS; the raster kernel declares it __shared__.
  struct Chunk {
    float4 seg[CHUNK];   // (ax, ay, bx - ax, by - ay) relative to the caller's origin
    float inv[CHUNK];    // 1 / |b - a|^2, 0 for a zero-length segment (a point)
    int cnt[WAVES];
  };

  // Compacts the segments the threads keep into the chunk, in thread order (ballot + popcount); s = this thread's segment as
  // the chunk holds it, read only where keep.  Returns how many were kept.  Ends on a barrier: the chunk can be read.
  static __device__ __forceinline__ int compact(Chunk& ch, bool keep, const float4& s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) ch.cnt[wave] = __popcll(vote);
    __syncthreads();
    int off = __popcll(vote & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) off += ch.cnt[w];
      kept += ch.cnt[w];
    }
    if (keep) {
      const float len2 = s.z * s.z + s.w * s.w;
      ch.seg[off] = s;
      ch.inv[off] = len2 > 0.f ? 1.f / len2 : 0.f;
    }
    __syncthreads();
    return kept;
  }

  // The running minima of the squared distance from this lane's pixel centres to the first `kept` segments of the chunk.
  // cx = the centre of the lane's first pixel and row = its row in the first pass, both relative to the chunk's origin.
  static __device__ __forceinline__ void min_dist2(const Chunk& ch, int kept, float cx, int row, int npass, float (&mn)[PASSES][4]) {
    for (int k = 0; k < kept; ++k) {
      const float4 a = ch.seg[k];   // every lane reads the same address: an LDS broadcast
      const float inv = ch.inv[k];
      float dx[4], dxab[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        dx[q] = cx + (float)q - a.x;
        dxab[q] = dx[q] * a.z;
      }
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        if (p >= npass) break;
        const float dy = (float)(row + p * ROWS_PER_PASS) + 0.5f - a.y;
        const float dyab = dy * a.w;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float t = fminf(fmaxf((dxab[q] + dyab) * inv, 0.f), 1.f);
          const float ex = dx[q] - t * a.z, ey = dy - t * a.w;
          mn[p][q] = fminf(mn[p][q], ex * ex + ey * ey);
        }
      }
    }
  }

  // img = one H x W image; row = this lane's image row in the first pass, col = its first column
  static __device__ __forceinline__ void store_coverage(float* img, int row, int col, int H, int W, float radius,
                                                        const float (&mn)[PASSES][4]) {
    if (col >= W) return;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = row + p * ROWS_PER_PASS;
      if (r < H) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float cov = fminf(fmaxf(radius - sqrtf(mn[p][q]), 0.f), 1.f);
          v[q] = 255.f * (1.f - cov);
        }
        *reinterpret_cast<float4*>(img + (size_t)r * W + col) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }

  static __device__ __forceinline__ void store_white(float* img, int row, int col, int H, int W) {
    if (col >= W) return;
    const float4 white = make_float4(255.f, 255.f, 255.f, 255.f);
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = row + p * ROWS_PER_PASS;
      if (r < H) *reinterpret_cast<float4*>(img + (size_t)r * W + col) = white;
    }
  }
};
