// paths.hip — the vector twin of the page compositor (include/dhw.h: dhw_paths): N sampled lines [N,L,3] -> the
// pen-down polylines of every line in page pixels, at the ONE scale and in the slots of dhw_page, smoothed, thinned, with a
// tangent per point, compacted in stroke order.  Two kernels, one workgroup of 256 threads per line, 16 strokes per thread:
//   paths_limits_kernel  the scan of the line rasteriser (render/line_raster.h) and s_n, the largest scale at which the line
//                        fits its slot.  Skipped when the caller gives the scale.
//   paths_kernel         s = min s_n over all lines, the same scan again (positions with the raster's bits stay in
//                        registers), then placement, smoothing, thinning, tangents and the compacted store.
// A thread owns positions 16 t .. 16 t + 15 from the scan to the store; what changes from round to round is a 16-bit mask of
// the points it still keeps.  What a thread needs of the others travels through ~6 KB of LDS per round: the drawn bit of the
// next thread's first segment; the count of kept points before it (wave scan + per-wave totals); its nearest kept
// neighbours left and right, found with a ballot of "keeps a point" per wave and clz / ffs over the four masks (after r
// rounds a neighbour may sit up to 2^r positions away, several threads off); and the rank of its polyline's start, from the
// nearest thread to the left that keeps a start.  No atomics, one writer per output element, nothing depends on the batch.
#include "../render/line_raster.h"
#include "paths.h"

// rules 4-7: every difference, product and sum is an fp32 operation of its own (hipcc contracts a * b + c by default)
#pragma clang fp contract(off)

namespace {

using LR = LineRaster<PATHS_THREADS, PATHS_ITEMS, PAGE_TILE_W, PAGE_BAND_H, PATHS_THREADS>;   // (only its scan is used)
constexpr int WAVES = PATHS_THREADS / 64;
constexpr unsigned ALL = (1u << PATHS_ITEMS) - 1u;

__device__ __forceinline__ bool takes_part(int total, int slot, long long nslots) { return total > 0 && slot >= 0 && (long long)slot < nslots; }

__global__ __launch_bounds__(PATHS_THREADS) void paths_limits_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                                     const int32_t* __restrict__ slots, int L, long long nslots, float pitch,
                                                                     float availw, float* __restrict__ sn_out) {
  const int b = blockIdx.x;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);   // (the API documents 1 <= n <= L; a bad device-side entry must not read out of bounds)
  LR::Scan sc;
  LR::scan(strokes + (size_t)b * L * 3, n, sc);
  if (threadIdx.x) return;
  float sn = __builtin_inff();
  if (takes_part(sc.total, slots ? slots[b] : b, nslots)) {
    const float ex = sc.xmax - sc.xmin, ey = sc.ymax - sc.ymin;
    if (ey > 0.f) sn = pitch / ey;   // one fp32 division each, as the page compositor's
    if (ex > 0.f) sn = fminf(sn, availw / ex);
  }
  sn_out[b] = sn;
}

// What a thread learns of the other threads' kept points in one exchange.
struct Around {
  int base, total;       // kept points of the threads before this one, and of the line
  int start_rank;        // the index among the line's kept points of the last start a thread before this one keeps (-1: none)
  float ax, ay, bx, by;  // the last kept point before this thread's and the first after them (0 where there is none)
};

struct Exchange {
  int cnt[WAVES];
  unsigned long long anyk[WAVES], anys[WAVES];   // per wave: which threads keep a point / keep a start
  int srank[PATHS_THREADS];                      // valid where the thread keeps a start
  float first[PATHS_THREADS][2], last[PATHS_THREADS][2];   // valid where the thread keeps a point
};

// the nearest thread before / after `tid` whose bit is set in the per-wave masks, -1 if none
__device__ __forceinline__ int prev_set(const unsigned long long* m, int wave, int lane) {
  unsigned long long bits = m[wave] & ((1ull << lane) - 1ull);
  int w = wave;
  while (!bits && w > 0) bits = m[--w];
  return bits ? w * 64 + 63 - __clzll((long long)bits) : -1;
}
__device__ __forceinline__ int next_set(const unsigned long long* m, int wave, int lane) {
  unsigned long long bits = m[wave] & ~((2ull << lane) - 1ull);   // (lane 63: 2 << 63 wraps to 0, the mask is empty)
  int w = wave;
  while (!bits && w < WAVES - 1) bits = m[++w];
  return bits ? w * 64 + __ffsll((long long)bits) - 1 : -1;
}

// kept / start: this thread's masks; x, y: its points.  Three barriers; the last one frees `e` for the next exchange.
__device__ __forceinline__ Around exchange(Exchange& e, unsigned kept, unsigned start, const float (&x)[PATHS_ITEMS], const float (&y)[PATHS_ITEMS]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = __popc(kept);
  const unsigned ks = kept & start;
  const int inc = wave_incl_scan(cnt, lane);
  const unsigned long long vk = __ballot(cnt != 0), vs = __ballot(ks != 0);
  if (lane == 63) e.cnt[wave] = inc;
  if (lane == 0) {
    e.anyk[wave] = vk;
    e.anys[wave] = vs;
  }
  float fx = 0.f, fy = 0.f, lx = 0.f, ly = 0.f;   // (selects over the unrolled items: the points stay in registers)
#pragma unroll
  for (int j = 0; j < PATHS_ITEMS; ++j) {
    if ((kept >> j) & 1u) {
      lx = x[j];
      ly = y[j];
    }
    if ((kept >> (PATHS_ITEMS - 1 - j)) & 1u) {
      fx = x[PATHS_ITEMS - 1 - j];
      fy = y[PATHS_ITEMS - 1 - j];
    }
  }
  e.first[tid][0] = fx;
  e.first[tid][1] = fy;
  e.last[tid][0] = lx;
  e.last[tid][1] = ly;
  __syncthreads();
  Around r;
  r.base = inc - cnt;
  r.total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) r.base += e.cnt[w];
    r.total += e.cnt[w];
  }
  // the index among the line's kept points of this thread's last kept start
  if (ks) e.srank[tid] = r.base + __popc(kept & ((1u << (31 - __clz(ks))) - 1u));
  __syncthreads();
  const int qa = prev_set(e.anyk, wave, lane), qb = next_set(e.anyk, wave, lane), qs = prev_set(e.anys, wave, lane);
  r.ax = qa >= 0 ? e.last[qa][0] : 0.f;
  r.ay = qa >= 0 ? e.last[qa][1] : 0.f;
  r.bx = qb >= 0 ? e.first[qb][0] : 0.f;
  r.by = qb >= 0 ? e.first[qb][1] : 0.f;
  r.start_rank = qs >= 0 ? e.srank[qs] : -1;
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(PATHS_THREADS) void paths_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                              const int32_t* __restrict__ slots, int N, int L, long long nslots, int lpp,
                                                              float margin_left, float margin_top, float pitch, float scale, int smooth, float tol2,
                                                              int rounds, const float* __restrict__ sn, float4* __restrict__ points_out,
                                                              int32_t* __restrict__ index_out, int32_t* __restrict__ counts_out,
                                                              float* __restrict__ scale_out, float* __restrict__ boxes_out) {
  __shared__ Exchange s_ex;
  __shared__ unsigned s_drawn[PATHS_THREADS];
  __shared__ int s_pcnt[WAVES];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);

  LR::Scan sc;
  LR::scan(strokes + (size_t)b * L * 3, n, sc);

  // the shared scale: the exact min of s_n over all lines (+inf where a line takes no part).  Every wave of every workgroup
  // reads all of them, 64 at a time, and gets the same bits, whatever the order.
  float s = scale;
  if (!(scale > 0.f)) {
    float m = __builtin_inff();
    for (int k = lane; k < N; k += 64) m = fminf(m, sn[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fminf(m, __shfl_xor(m, d));
    s = m < __builtin_inff() ? m : 1.f;
  }
  if (b == 0 && tid == 0) *scale_out = s;

  float4* pts = points_out + (size_t)b * L;
  int32_t* idx = index_out + (size_t)b * L * 2;
  const int slot = slots ? slots[b] : b;
  if (!takes_part(sc.total, slot, nslots)) {   // (workgroup-uniform) no path: counts (0, 0), a zero box, every row empty
    for (int k = tid; k < L; k += PATHS_THREADS) {
      pts[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      idx[2 * k] = -1;
      idx[2 * k + 1] = -1;
    }
    if (tid < 2) counts_out[2 * b + tid] = 0;
    if (tid < 4) boxes_out[4 * b + tid] = 0.f;
    return;
  }

  // rule 3: position i is a point iff segment i or i + 1 is drawn; it starts a polyline iff segment i is not, ends one iff
  // segment i + 1 is not.  Segment 16 t + 16 belongs to the next thread.
  s_drawn[tid] = sc.drawn;
  __syncthreads();
  const unsigned dnext = ((sc.drawn >> 1) | ((tid + 1 < PATHS_THREADS ? s_drawn[tid + 1] & 1u : 0u) << (PATHS_ITEMS - 1))) & ALL;
  const unsigned point = sc.drawn | dnext, start = point & ~sc.drawn, end = point & ~dnext, inner = sc.drawn & dnext;

  // polylines before this thread's first start, and of the line
  const int pmine = __popc(start), pinc = wave_incl_scan(pmine, lane);
  if (lane == 63) s_pcnt[wave] = pinc;
  __syncthreads();
  int pbase = pinc - pmine, ptotal = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) pbase += s_pcnt[w];
    ptotal += s_pcnt[w];
  }

  // rule 4: placement
  const float ex = sc.xmax - sc.xmin, ey = sc.ymax - sc.ymin;
  const float top = margin_top + (float)(slot % lpp) * pitch;
  const float oy = top + (pitch - ey * s) * 0.5f;
  float x[PATHS_ITEMS], y[PATHS_ITEMS];
#pragma unroll
  for (int j = 0; j < PATHS_ITEMS; ++j) {
    x[j] = margin_left + (sc.px[j] - sc.xmin) * s;
    y[j] = oy + (sc.ymax - sc.py[j]) * s;
  }
  if (tid == 0) {   // rule 9
    boxes_out[4 * b] = margin_left;
    boxes_out[4 * b + 1] = oy;
    boxes_out[4 * b + 2] = margin_left + ex * s;
    boxes_out[4 * b + 3] = oy + ey * s;
  }

  // rule 5: smoothing.  The neighbours of an inner point are positions i - 1 and i + 1; across a thread boundary they are the
  // neighbouring thread's last / first position.
  for (int p = 0; p < smooth; ++p) {
    s_ex.first[tid][0] = x[0];
    s_ex.first[tid][1] = y[0];
    s_ex.last[tid][0] = x[PATHS_ITEMS - 1];
    s_ex.last[tid][1] = y[PATHS_ITEMS - 1];
    __syncthreads();
    const float lx = tid ? s_ex.last[tid - 1][0] : 0.f, ly = tid ? s_ex.last[tid - 1][1] : 0.f;
    const float rx = tid + 1 < PATHS_THREADS ? s_ex.first[tid + 1][0] : 0.f, ry = tid + 1 < PATHS_THREADS ? s_ex.first[tid + 1][1] : 0.f;
    __syncthreads();
    float nx[PATHS_ITEMS], ny[PATHS_ITEMS];
#pragma unroll
    for (int j = 0; j < PATHS_ITEMS; ++j) {
      const float x0 = j ? x[j - 1] : lx, x1 = j + 1 < PATHS_ITEMS ? x[j + 1] : rx;
      const float y0 = j ? y[j - 1] : ly, y1 = j + 1 < PATHS_ITEMS ? y[j + 1] : ry;
      const bool in = (inner >> j) & 1u;
      nx[j] = in ? (x0 + x1) * 0.25f + x[j] * 0.5f : x[j];
      ny[j] = in ? (y0 + y1) * 0.25f + y[j] * 0.5f : y[j];
    }
#pragma unroll
    for (int j = 0; j < PATHS_ITEMS; ++j) {
      x[j] = nx[j];
      y[j] = ny[j];
    }
  }

  // rule 6: thinning.  Every decision of a round reads the masks and neighbours of its start; points never move.
  unsigned kept = point;
  for (int r = 0; r < rounds; ++r) {
    const Around a = exchange(s_ex, kept, start, x, y);
    // forward: the previous kept neighbour of every kept point, and whether its rank in its polyline is odd
    float pax[PATHS_ITEMS], pay[PATHS_ITEMS];
    unsigned odd = 0;
    {
      int k = a.base, ks = a.start_rank;
      float ax = a.ax, ay = a.ay;
#pragma unroll
      for (int j = 0; j < PATHS_ITEMS; ++j) {
        pax[j] = ax;
        pay[j] = ay;
        if ((kept >> j) & 1u) {
          if ((start >> j) & 1u) ks = k;
          if ((k - ks) & 1) odd |= 1u << j;
          ax = x[j];
          ay = y[j];
          ++k;
        }
      }
    }
    // backward: the next kept neighbour, and the decision
    const unsigned cand = kept & odd & ~end;
    unsigned removed = 0;
    float bx = a.bx, by = a.by;
#pragma unroll
    for (int j = PATHS_ITEMS - 1; j >= 0; --j) {
      if ((cand >> j) & 1u) {
        const float abx = bx - pax[j], aby = by - pay[j], apx = x[j] - pax[j], apy = y[j] - pay[j];
        const float len2 = abx * abx + aby * aby;
        float d2;
        if (len2 == 0.f) {
          d2 = apx * apx + apy * apy;
        } else {
          const float t = fminf(fmaxf((apx * abx + apy * aby) / len2, 0.f), 1.f);
          const float dx = apx - t * abx, dy = apy - t * aby;
          d2 = dx * dx + dy * dy;
        }
        if (d2 <= tol2) removed |= 1u << j;
      }
      if ((kept >> j) & 1u) {
        bx = x[j];
        by = y[j];
      }
    }
    kept &= ~removed;
  }

  // rules 7, 8: tangents from the kept neighbours inside the polyline, and the compacted store
  const Around a = exchange(s_ex, kept, start, x, y);
  float pax[PATHS_ITEMS], pay[PATHS_ITEMS];
  {
    float ax = a.ax, ay = a.ay;
#pragma unroll
    for (int j = 0; j < PATHS_ITEMS; ++j) {
      pax[j] = ax;
      pay[j] = ay;
      if ((kept >> j) & 1u) {
        ax = x[j];
        ay = y[j];
      }
    }
  }
  {
    float bx = a.bx, by = a.by;
#pragma unroll
    for (int j = PATHS_ITEMS - 1; j >= 0; --j) {
      if ((kept >> j) & 1u) {
        const bool st = (start >> j) & 1u, en = (end >> j) & 1u;
        const float px = st ? x[j] : pax[j], py = st ? y[j] : pay[j];
        const float qx = en ? x[j] : bx, qy = en ? y[j] : by;
        const int k = a.base + __popc(kept & ((1u << j) - 1u));
        pts[k] = make_float4(x[j], y[j], (qx - px) / 6.0f, (qy - py) / 6.0f);
        idx[2 * k] = tid * PATHS_ITEMS + j;
        idx[2 * k + 1] = pbase + __popc(start & ((2u << j) - 1u)) - 1;
        bx = x[j];
        by = y[j];
      }
    }
  }
  for (int k = a.total + tid; k < L; k += PATHS_THREADS) {
    pts[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    idx[2 * k] = -1;
    idx[2 * k + 1] = -1;
  }
  if (tid == 0) {
    counts_out[2 * b] = a.total;
    counts_out[2 * b + 1] = ptotal;
  }
}

}  // namespace

hipError_t launch_paths_limits(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, const PageGeometry& g, float* sn,
                               hipStream_t st) {
  const long long nslots = (long long)g.P * g.lines_per_page;
  const float availw = (float)g.W - 2.f * g.margin_left;
  hipLaunchKernelGGL(paths_limits_kernel, dim3(N), dim3(PATHS_THREADS), 0, st, strokes, lens, slots, L, nslots, g.pitch, availw, sn);
  return hipGetLastError();
}

hipError_t launch_paths(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, const PageGeometry& g, const PathsOptions& o,
                        const float* sn, const PathsOut& out, hipStream_t st) {
  const long long nslots = (long long)g.P * g.lines_per_page;
  const float tol2 = o.tol * o.tol;
  hipLaunchKernelGGL(paths_kernel, dim3(N), dim3(PATHS_THREADS), 0, st, strokes, lens, slots, N, L, nslots, g.lines_per_page, g.margin_left,
                     g.margin_top, g.pitch, g.scale, o.smooth, tol2, o.rounds, sn, out.points, out.index, out.counts, out.scale, out.boxes);
  return hipGetLastError();
}
