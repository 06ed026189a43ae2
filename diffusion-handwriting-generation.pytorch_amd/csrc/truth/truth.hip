// truth.hip — ground truth for written pages (include/dhw.h: dhw_truth): N sampled lines [N,L,3] and the group
// of every stroke row [N,L] -> the box and the row span of every group in page pixels, at the ONE scale and in the slots of
// dhw_page, and a per-pixel map of which group's ink is nearest.  Three kernels:
//   truth_prepare_kernel  one workgroup per line: the scan of the line rasteriser (render/line_raster.h), s_n, every group's
//                         span and box (runs of one group reduced in registers, then LDS integer min / max on an
//                         order-preserving image of the float: exact and commutative), and, for the label map, the drawn
//                         segments relative to the box corner with their ids, compacted in stroke order into the workspace.
//                         With the caller's scale the boxes are placed here.
//   truth_place_kernel    automatic scale only: s = min s_n over the headers, then one thread per group places its box.
//   truth_label_kernel    one workgroup per (page, 32-column tile, 96-row band), as page_raster_kernel: the lines that reach
//                         the tile, their segments culled into a labelled LDS chunk, and per pixel the lexicographic minimum
//                         of (squared distance, id) over all of them.
// No global atomics, no float atomics, one writer per output element: nothing depends on the order of the lines.
#include "../render/line_raster.h"
#include "truth.h"

// rule 3: every difference, product and sum of the boxes is an fp32 operation of its own (hipcc contracts a * b + c by default)
#pragma clang fp contract(off)

namespace {

using LR = LineRaster<TRUTH_THREADS, PAGE_ITEMS, PAGE_TILE_W, PAGE_BAND_H, PAGE_CHUNK>;

// an unsigned image of a float with the same order (no NaN reaches it: positions are sums of the finite input).  It ranks
// -0.0 below +0.0, which fminf does not; no position is -0.0: the scan's sums start at +0.0, and in round-to-nearest a sum is
// -0.0 only when both terms are.  The runs start at +-3.0e38f, the sentinels of the scan's own line box: a group box and
// the line box agree on every input, also on one beyond that magnitude.
__device__ __forceinline__ unsigned ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? u & 0x7fffffffu : ~u); }

// the shared scale: the exact min of s_n over the lines that draw, 1 if none is finite.  Every wave reads all headers (64 at
// a time, no barrier) and gets the same bits, whatever the order.
__device__ __forceinline__ float shared_scale(const PageLineHeader* __restrict__ hdr, int N, int lane) {
  float m = __builtin_inff();
  for (int n = lane; n < N; n += 64)
    if (hdr[n].count > 0) m = fminf(m, hdr[n].s_n);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fminf(m, __shfl_xor(m, d));
  return m < __builtin_inff() ? m : 1.f;
}

// rule 3: a group's box (gxmin, gymax, gxmax, gymin in stroke units) on the page -> (left, top, right, bottom)
__device__ __forceinline__ float4 place_group(const float4& raw, float xmin, float ymax, float ey, int slot, int lpp, float margin_left,
                                              float margin_top, float pitch, float s) {
  const float top = margin_top + (float)(slot % lpp) * pitch;
  const float oy = top + (pitch - ey * s) * 0.5f;
  return make_float4(margin_left + (raw.x - xmin) * s, oy + (ymax - raw.y) * s, margin_left + (raw.z - xmin) * s, oy + (ymax - raw.w) * s);
}

// one run of consecutive drawn segments of one group, in a thread's registers
struct Run {
  int g, first, last, cnt;
  float xmin, xmax, ymin, ymax;
};

struct GroupTable {   // 7 KB next to the scan's 50 KB
  unsigned xmin[TRUTH_MAX_G], xmax[TRUTH_MAX_G], ymin[TRUTH_MAX_G], ymax[TRUTH_MAX_G];
  int first[TRUTH_MAX_G], last[TRUTH_MAX_G], cnt[TRUTH_MAX_G];
};

__device__ __forceinline__ void flush(GroupTable& t, const Run& r) {
  if (r.cnt == 0) return;   // (r.g lies in [0, G) whenever cnt > 0)
  atomicMin(&t.xmin[r.g], ordered(r.xmin));
  atomicMax(&t.xmax[r.g], ordered(r.xmax));
  atomicMin(&t.ymin[r.g], ordered(r.ymin));
  atomicMax(&t.ymax[r.g], ordered(r.ymax));
  atomicMin(&t.first[r.g], r.first);
  atomicMax(&t.last[r.g], r.last);
  atomicAdd(&t.cnt[r.g], r.cnt);
}

__global__ __launch_bounds__(TRUTH_THREADS) void truth_prepare_kernel(const float* __restrict__ strokes, const int32_t* __restrict__ lens,
                                                                      const int32_t* __restrict__ slots, const int32_t* __restrict__ groups, int L,
                                                                      int G, long long nslots, int lpp, float margin_left, float margin_top,
                                                                      float pitch, float availw, float scale, int want_segs,
                                                                      PageLineHeader* __restrict__ hdr, float4* __restrict__ segs,
                                                                      int32_t* __restrict__ ids, float* __restrict__ boxes_out,
                                                                      int32_t* __restrict__ spans_out, float* __restrict__ scale_out) {
  __shared__ GroupTable s_tab;

  const int b = blockIdx.x, tid = threadIdx.x;
  int n = lens ? lens[b] : L;
  n = min(max(n, 0), L);   // (the API documents 1 <= n <= L; a bad device-side entry must not read out of bounds)

  if (tid < G) {   // (G <= TRUTH_THREADS; the barriers of the scan stand between this and the first flush)
    s_tab.xmin[tid] = s_tab.ymin[tid] = 0xffffffffu;
    s_tab.xmax[tid] = s_tab.ymax[tid] = 0u;
    s_tab.first[tid] = 0x7fffffff;
    s_tab.last[tid] = -1;
    s_tab.cnt[tid] = 0;
  }

  LR::Scan sc;
  LR::scan(strokes + (size_t)b * L * 3, n, sc);

  float* bo = boxes_out + (size_t)b * G * 4;
  int32_t* so = spans_out + (size_t)b * G * 3;
  if (b == 0 && tid == 0 && scale > 0.f) *scale_out = scale;

  const int slot = slots ? slots[b] : b;
  if (sc.total == 0 || slot < 0 || (long long)slot >= nslots) {   // (workgroup-uniform) takes no part: rule 5
    if (tid == 0) hdr[b] = PageLineHeader{0, 0.f, 0.f, 0.f, 0.f, __builtin_inff(), slot, 0};
    if (tid < G) {
      float* o = bo + 4 * tid;
      o[0] = o[1] = o[2] = o[3] = 0.f;
      so[3 * tid] = so[3 * tid + 1] = so[3 * tid + 2] = 0;
    }
    return;
  }

  const float ex = sc.xmax - sc.xmin, ey = sc.ymax - sc.ymin;
  if (tid == 0) {
    float sn = __builtin_inff();
    if (ey > 0.f) sn = pitch / ey;   // one fp32 division each, as the page compositor's
    if (ex > 0.f) sn = fminf(sn, availw / ex);
    hdr[b] = PageLineHeader{sc.total, sc.xmin, sc.ymax, ex, ey, sn, slot, 0};
  }

  // a drawn segment i has 1 <= i < last < n <= L: its group is inside row b of `groups`, its place inside row b of the workspace
  const int32_t* gr = groups + (size_t)b * L + tid * PAGE_ITEMS;
  float4* oseg = segs + (size_t)b * L + sc.off;
  int32_t* oid = ids + (size_t)b * L + sc.off;
  Run run{-1, 0, 0, 0, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < PAGE_ITEMS; ++j) {
    if ((sc.drawn >> j) & 1u) {
      const int g = gr[j];
      const bool assigned = (unsigned)g < (unsigned)G;   // rule 2
      const float ax = sc.ax(j), ay = sc.ay(j), bx = sc.px[j], by = sc.py[j];
      if (want_segs) {
        *oseg++ = make_float4(ax - sc.xmin, sc.ymax - ay, bx - sc.xmin, sc.ymax - by);   // y flipped: image rows go down
        *oid++ = assigned ? 1 + b * G + g : 0;
      }
      if (assigned) {
        if (g != run.g) {
          flush(s_tab, run);
          run = Run{g, tid * PAGE_ITEMS + j, 0, 0, 3.0e38f, -3.0e38f, 3.0e38f, -3.0e38f};
        }
        run.last = tid * PAGE_ITEMS + j;
        ++run.cnt;
        run.xmin = fminf(run.xmin, fminf(ax, bx));
        run.xmax = fmaxf(run.xmax, fmaxf(ax, bx));
        run.ymin = fminf(run.ymin, fminf(ay, by));
        run.ymax = fmaxf(run.ymax, fmaxf(ay, by));
      }
    }
  }
  flush(s_tab, run);
  __syncthreads();

  if (tid < G) {
    const int cnt = s_tab.cnt[tid];
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    int first = 0, end = 0;
    if (cnt > 0) {   // rules 3, 4
      first = s_tab.first[tid];
      end = s_tab.last[tid] + 1;
      box = make_float4(unordered(s_tab.xmin[tid]), unordered(s_tab.ymax[tid]), unordered(s_tab.xmax[tid]), unordered(s_tab.ymin[tid]));
      if (scale > 0.f) box = place_group(box, sc.xmin, sc.ymax, ey, slot, lpp, margin_left, margin_top, pitch, scale);
    }
    float* o = bo + 4 * tid;
    o[0] = box.x;
    o[1] = box.y;
    o[2] = box.z;
    o[3] = box.w;
    so[3 * tid] = first;
    so[3 * tid + 1] = end;
    so[3 * tid + 2] = cnt;
  }
}

__global__ __launch_bounds__(TRUTH_THREADS) void truth_place_kernel(const PageLineHeader* __restrict__ hdr, int N, int G, int lpp, float margin_left,
                                                                    float margin_top, float pitch, float* __restrict__ boxes_out,
                                                                    const int32_t* __restrict__ spans_out, float* __restrict__ scale_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float s = shared_scale(hdr, N, tid & 63);
  if (b == 0 && tid == 0) *scale_out = s;
  const PageLineHeader h = hdr[b];
  if (h.count <= 0 || tid >= G) return;                          // (zeros already)
  if (spans_out[((size_t)b * G + tid) * 3 + 2] <= 0) return;     // (zeros already)
  float* o = boxes_out + ((size_t)b * G + tid) * 4;
  const float4 box = place_group(make_float4(o[0], o[1], o[2], o[3]), h.xmin, h.ymax, h.ey, h.slot, lpp, margin_left, margin_top, pitch, s);
  o[0] = box.x;
  o[1] = box.y;
  o[2] = box.z;
  o[3] = box.w;
}

// From here on the arithmetic is the page compositor's (page/page.hip is compiled with the default contraction): rule 7 asks
// for its placement of the segments and its distance, not for the boxes' unfused operations.
#pragma clang fp contract(fast)

// where a line's ink box lands on its page at scale s (page.hip: place_line)
__device__ __forceinline__ float4 place_line(const PageLineHeader& h, float s, int lpp, float margin_left, float margin_top, float pitch) {
  const float top = margin_top + (float)(h.slot % lpp) * pitch;
  const float oy = top + (pitch - h.ey * s) * 0.5f;
  return make_float4(margin_left, oy, margin_left + h.ex * s, oy + h.ey * s);
}

// LineRaster::Chunk with an id per segment
struct LabelChunk {
  float4 seg[PAGE_CHUNK];   // (ax, ay, bx - ax, by - ay) relative to the origin of the tile and band
  float inv[PAGE_CHUNK];    // 1 / |b - a|^2, 0 for a zero-length segment (a point)
  int id[PAGE_CHUNK];
  int cnt[LR::WAVES];
};

// LineRaster::compact with the id carried along: thread order, ballot + popcount.  Ends on a barrier.
__device__ __forceinline__ int compact_labelled(LabelChunk& ch, bool keep, const float4& s, int id) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long vote = __ballot(keep);
  if (lane == 0) ch.cnt[wave] = __popcll(vote);
  __syncthreads();
  int off = __popcll(vote & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
  for (int w = 0; w < LR::WAVES; ++w) {
    if (w < wave) off += ch.cnt[w];
    kept += ch.cnt[w];
  }
  if (keep) {   // (off < kept <= PAGE_CHUNK = the number of threads)
    const float len2 = s.z * s.z + s.w * s.w;
    ch.seg[off] = s;
    ch.inv[off] = len2 > 0.f ? 1.f / len2 : 0.f;
    ch.id[off] = id;
  }
  __syncthreads();
  return kept;
}

// LineRaster::min_dist2 in its tile-relative form, with the running lexicographic minimum of (d2, id)
__device__ __forceinline__ void min_labelled(const LabelChunk& ch, int kept, float cx, int row, int npass, float (&mn)[LR::PASSES][4],
                                             int (&who)[LR::PASSES][4]) {
  for (int k = 0; k < kept; ++k) {
    const float4 a = ch.seg[k];   // every lane reads the same address: an LDS broadcast
    const float inv = ch.inv[k];
    const int id = ch.id[k];
    float dx[4], dxab[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      dx[q] = cx + (float)q - a.x;
      dxab[q] = dx[q] * a.z;
    }
#pragma unroll
    for (int p = 0; p < LR::PASSES; ++p) {
      if (p >= npass) break;
      const float dy = (float)(row + p * LR::ROWS_PER_PASS) + 0.5f - a.y;
      const float dyab = dy * a.w;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float t = fminf(fmaxf((dxab[q] + dyab) * inv, 0.f), 1.f);
        const float ex = dx[q] - t * a.z, ey = dy - t * a.w;
        const float d2 = ex * ex + ey * ey;
        const bool less = d2 < mn[p][q] || (d2 == mn[p][q] && id < who[p][q]);
        mn[p][q] = less ? d2 : mn[p][q];
        who[p][q] = less ? id : who[p][q];
      }
    }
  }
}

__global__ __launch_bounds__(TRUTH_THREADS) void truth_label_kernel(const PageLineHeader* __restrict__ hdr, const float4* __restrict__ segs,
                                                                    const int32_t* __restrict__ ids, int N, int L, int tiles, int H, int W, int lpp,
                                                                    float margin_left, float margin_top, float pitch, float line_width,
                                                                    float scale, int32_t* __restrict__ labels) {
  __shared__ LabelChunk s_chunk;
  __shared__ int s_line[TRUTH_THREADS];   // the lines of one header round that reach this tile, in line order
  __shared__ int s_lcnt[LR::WAVES];

  const int p = blockIdx.x / tiles, tile = blockIdx.x - p * tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = tile * PAGE_TILE_W, y0 = blockIdx.z * PAGE_BAND_H;
  const int lx = tid % LR::LANES_X;
  const int col = x0 + 4 * lx;
  const int rloc = tid / LR::LANES_X;   // this lane's row in the first pass, relative to the band
  int32_t* out = labels + (size_t)p * H * W;

  const float s = scale > 0.f ? scale : shared_scale(hdr, N, lane);

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

  bool any = false;   // (per wave, and the same in every wave: the exit below needs no barrier)
  for (int nb = 0; nb < N && !any; nb += 64) any = __ballot(reaches(nb + lane)) != 0ull;
  if (!any) {   // no ink near: all 0
    if (col < W) {
#pragma unroll
      for (int q = 0; q < LR::PASSES; ++q) {
        const int r = y0 + rloc + q * LR::ROWS_PER_PASS;
        if (r < H) *reinterpret_cast<int4*>(out + (size_t)r * W + col) = make_int4(0, 0, 0, 0);
      }
    }
    return;
  }

  const float cx = (float)(4 * lx) + 0.5f;   // centre of this lane's first pixel, relative to the tile origin
  const int npass = min(LR::PASSES, (H - y0 + LR::ROWS_PER_PASS - 1) / LR::ROWS_PER_PASS);

  float mn[LR::PASSES][4];
  int who[LR::PASSES][4];
#pragma unroll
  for (int q = 0; q < LR::PASSES; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mn[q][k] = 1.0e30f;
      who[q][k] = 0;
    }

  for (int nb = 0; nb < N; nb += TRUTH_THREADS) {
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
      const int ln = s_line[hl];   // every lane reads the same address
      const PageLineHeader h = hdr[ln];
      const float4 box = place_line(h, s, lpp, margin_left, margin_top, pitch);
      const float ox = box.x, oy = box.y;
      const float4* rs = segs + (size_t)ln * L;
      const int32_t* ri = ids + (size_t)ln * L;
      for (int base = 0; base < h.count; base += PAGE_CHUNK) {   // (h.count <= L: the prepare kernel counted drawn rows)
        const int j = base + tid;
        bool keep = false;
        int id = 0;
        float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
        if (j < h.count) {
          const float4 r = rs[j];
          id = ri[j];
          ax = ox + r.x * s;
          ay = oy + r.y * s;
          bx = ox + r.z * s;
          by = oy + r.w * s;
          keep = fminf(ax, bx) < thi && fmaxf(ax, bx) > tlo && fminf(ay, by) < bhi && fmaxf(ay, by) > blo;
        }
        const int kept = compact_labelled(s_chunk, keep, make_float4(ax - (float)x0, ay - (float)y0, bx - ax, by - ay), id);
        min_labelled(s_chunk, kept, cx, rloc, npass, mn, who);
        __syncthreads();   // the next round overwrites the chunk
      }
    }
    __syncthreads();   // the next header round overwrites the line list
  }

  if (col < W) {
#pragma unroll
    for (int q = 0; q < LR::PASSES; ++q) {
      const int r = y0 + rloc + q * LR::ROWS_PER_PASS;
      if (r < H) {
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = sqrtf(mn[q][k]) < radius ? who[q][k] : 0;
        *reinterpret_cast<int4*>(out + (size_t)r * W + col) = make_int4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

}  // namespace

hipError_t launch_truth_prepare(const float* strokes, const int32_t* lens, const int32_t* slots, const int32_t* groups, int N, int L, int G,
                                const PageGeometry& g, bool want_segs, const TruthWorkspace& w, float* boxes_out, int32_t* spans_out,
                                float* scale_out, hipStream_t st) {
  const long long nslots = (long long)g.P * g.lines_per_page;
  const float availw = (float)g.W - 2.f * g.margin_left;
  hipLaunchKernelGGL(truth_prepare_kernel, dim3(N), dim3(TRUTH_THREADS), 0, st, strokes, lens, slots, groups, L, G, nslots, g.lines_per_page,
                     g.margin_left, g.margin_top, g.pitch, availw, g.scale, want_segs ? 1 : 0, w.hdr, w.segs, w.ids, boxes_out, spans_out, scale_out);
  return hipGetLastError();
}

hipError_t launch_truth_place(int N, int G, const PageGeometry& g, const TruthWorkspace& w, float* boxes_out, const int32_t* spans_out,
                              float* scale_out, hipStream_t st) {
  hipLaunchKernelGGL(truth_place_kernel, dim3(N), dim3(TRUTH_THREADS), 0, st, w.hdr, N, G, g.lines_per_page, g.margin_left, g.margin_top, g.pitch,
                     boxes_out, spans_out, scale_out);
  return hipGetLastError();
}

hipError_t launch_truth_labels(int N, int L, const PageGeometry& g, const TruthWorkspace& w, int32_t* labels_out, hipStream_t st) {
  const int tiles = (g.W + PAGE_TILE_W - 1) / PAGE_TILE_W, bands = (g.H + PAGE_BAND_H - 1) / PAGE_BAND_H;
  hipLaunchKernelGGL(truth_label_kernel, dim3((unsigned)g.P * (unsigned)tiles, 1, bands), dim3(TRUTH_THREADS), 0, st, w.hdr, w.segs, w.ids, N, L,
                     tiles, g.H, g.W, g.lines_per_page, g.margin_left, g.margin_top, g.pitch, g.line_width, g.scale, labels_out);
  return hipGetLastError();
}
