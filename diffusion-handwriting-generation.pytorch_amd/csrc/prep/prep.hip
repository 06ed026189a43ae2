// prep.hip — writer-image preparation (include/dhw.h: dhw_prep): B grey images of different sizes, each in the
// top-left corner of its [Hin,Win] u8 slot -> one f32 [B,1,H,W] batch: cropped to the ink, resized to H rows by a fixed-point
// cubic, padded white to W.  Three launches on one stream, no host read in between:
//   init    the boxes int32 [B][4] in the workspace = (INT_MAX, -1, INT_MAX, -1)
//   box     grid (1024-column tile, 64-row strip, image): a lane loads 16 bytes of a row, masks the bytes at or past w and keeps
//           a 16-bit dark flag per column; a row is dark iff the wave's ballot of its masks is non-zero.  The wave's first / last
//           dark row and column meet in LDS, then one thread issues four integer atomicMin / atomicMax on the image's box.
//   resize  grid (256-column tile, 32-row band, image): the tile's x0 / cx and the band's y0 / cy are evaluated once (fp64, no
//           FMA) into LDS; a thread owns four adjacent output columns, takes their 4 x 4 taps straight from global memory
//           (one 16-byte window per source row where the taps fit one, else sixteen byte gathers; the crop is read through
//           the caches: neighbouring outputs share taps) and ends each row with one 16-byte store.  Columns at or past ow,
//           and whole images with a non-zero status, store 255.
// Integer min / max are exact and commutative and the resize is integer arithmetic on fixed coefficients: an image gives the
// same bits alone, in any batch, at any Hin, Win and W.
#include <climits>

#include "prep.h"

#pragma clang fp contract(off)

namespace {

constexpr int T = PREP_THREADS;

__global__ __launch_bounds__(T) void prep_init_kernel(int32_t* __restrict__ boxes, int B) {
  const int b = blockIdx.x * T + threadIdx.x;
  if (b < B) reinterpret_cast<int4*>(boxes)[b] = make_int4(INT_MAX, -1, INT_MAX, -1);
}

// (h, w) of image b; false (rule 4 bit 1) when it does not fit its slot: nothing of such an image is read
__device__ __forceinline__ bool image_size(const int32_t* __restrict__ sizes, int b, int Hin, int Win, int& h, int& w) {
  h = sizes ? sizes[2 * b] : Hin;
  w = sizes ? sizes[2 * b + 1] : Win;
  return h >= 1 && h <= Hin && w >= 1 && w <= Win;
}

// bit i = (byte i of the 16 < thresh); byte j of dword k is column 4k + j (little endian)
__device__ __forceinline__ unsigned dark16(const uint4& v, unsigned thresh) {
  const unsigned d[4] = {v.x, v.y, v.z, v.w};
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m |= (unsigned)(((d[k] >> (8 * j)) & 255u) < thresh) << (4 * k + j);
  return m;
}

__global__ __launch_bounds__(T) void prep_box_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ sizes, int Hin, int Win,
                                                     int thresh, int32_t* __restrict__ boxes) {
  __shared__ int s_box[4];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int h, w;
  if (!image_size(sizes, b, Hin, Win, h, w)) return;
  const int tile0 = blockIdx.x * PREP_BOX_COLS, strip0 = blockIdx.y * PREP_BOX_ROWS;
  if (strip0 >= h || tile0 >= w) return;   // (workgroup-uniform, as the return above)
  if (tid == 0) {
    s_box[0] = s_box[2] = INT_MAX;
    s_box[1] = s_box[3] = -1;
  }
  __syncthreads();

  // 16 * lane < w <= Win and Win % 16 == 0: the 16 bytes lie inside the row; those at or past w are masked out (rule 1)
  const int col0 = tile0 + 16 * lane;
  const bool live = col0 < w;
  const unsigned valid = !live ? 0u : (w - col0 >= 16 ? 0xFFFFu : (1u << (w - col0)) - 1u);
  const uint8_t* src = images + (size_t)b * Hin * Win + col0;
  constexpr int ROWS = PREP_BOX_ROWS / (T / 64);
  const int row0 = strip0 + wave * ROWS;
  unsigned colmask = 0;
  int rmin = INT_MAX, rmax = -1;
  for (int i = 0; i < ROWS; i += 4) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // four rows in flight; a row at or past h is skipped (white: never dark)
      const int r = row0 + i + u;
      v[u] = make_uint4(~0u, ~0u, ~0u, ~0u);
      if (live && r < h) v[u] = *reinterpret_cast<const uint4*>(src + (size_t)r * Win);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned m = dark16(v[u], (unsigned)thresh) & valid;
      colmask |= m;
      if (__ballot(m != 0)) {   // rows ascend: the first hit is the minimum, the latest the maximum
        rmin = min(rmin, row0 + i + u);
        rmax = row0 + i + u;
      }
    }
  }
  const unsigned long long nz = __ballot(colmask != 0);
  if (nz) {   // (wave-uniform)
    const int first = __ffsll(nz) - 1, last = 63 - __clzll((long long)nz);
    const unsigned mf = __shfl(colmask, first), ml = __shfl(colmask, last);
    if (lane == 0) {
      atomicMin(&s_box[0], rmin);
      atomicMax(&s_box[1], rmax);
      atomicMin(&s_box[2], tile0 + 16 * first + (__ffs(mf) - 1));
      atomicMax(&s_box[3], tile0 + 16 * last + (31 - __clz(ml)));
    }
  }
  __syncthreads();
  if (tid == 0 && s_box[1] >= 0) {
    atomicMin(&boxes[4 * b + 0], s_box[0]);
    atomicMax(&boxes[4 * b + 1], s_box[1]);
    atomicMin(&boxes[4 * b + 2], s_box[2]);
    atomicMax(&boxes[4 * b + 3], s_box[3]);
  }
}

// Rule 5 for destination sample d of an axis with n_in source and n_out destination samples: the first tap x0 - 1 and the
// four 11-bit coefficients.  (2d + 1) n_in <= 8191 * 16384 and x0 den <= 16384 * 8192: all within int32.
__device__ __forceinline__ void cubic_coef(int d, int n_in, int n_out, int& x0, int4& c) {
  const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;
  x0 = num >= 0 ? num / den : -((den - 1 - num) / den);   // floor
  const double t = (double)(num - x0 * den) / (double)den;
  const double a = -0.75, u = t + 1.0, s = 1.0 - t;
  const double w0 = ((a * u - 5.0 * a) * u + 8.0 * a) * u - 4.0 * a;
  const double w1 = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  const double w2 = ((a + 2.0) * s - (a + 3.0)) * s * s + 1.0;
  c.x = (int)rint(2048.0 * w0);
  c.y = (int)rint(2048.0 * w1);
  c.z = (int)rint(2048.0 * w2);
  c.w = 2048 - c.x - c.y - c.z;
}

__global__ __launch_bounds__(T) void prep_resize_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ sizes, int Hin, int Win,
                                                        int H, int W, const int32_t* __restrict__ boxes, float* __restrict__ img_out,
                                                        int32_t* __restrict__ widths_out, int32_t* __restrict__ boxes_out,
                                                        int32_t* __restrict__ status_out) {
  __shared__ int s_x0[PREP_TILE_COLS];
  __shared__ int4 s_cx[PREP_TILE_COLS];
  __shared__ int s_y0[PREP_BAND_ROWS];
  __shared__ int4 s_cy[PREP_BAND_ROWS];
  const int b = blockIdx.z, tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;

  // rules 2 to 4, the same in every thread of every workgroup of the image
  int h, w, r0 = 0, r1 = 0, c0 = 0, c1 = 0, ch = 0, cw = 0, ow = 0;
  int status = image_size(sizes, b, Hin, Win, h, w) ? 0 : 1;
  if (!status) {
    const int4 bx = reinterpret_cast<const int4*>(boxes)[b];
    if (bx.y < 0) {
      status = 2;
    } else {
      r0 = bx.x, r1 = bx.y, c0 = bx.z, c1 = bx.w;
      ch = r1 - r0, cw = c1 - c0;
      if (ch == 0 || cw == 0) {
        status = 2;
      } else {
        ow = H * cw / ch;   // H cw <= 512 * 16384
        if (ow > W) status = 4;
        if (ow == 0) status = 8;
      }
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    status_out[b] = status;
    if (widths_out) widths_out[b] = status ? 0 : ow;
    if (boxes_out) {
      boxes_out[4 * b + 0] = r0;
      boxes_out[4 * b + 1] = r1;
      boxes_out[4 * b + 2] = c0;
      boxes_out[4 * b + 3] = c1;
    }
  }

  const int tile0 = blockIdx.x * PREP_TILE_COLS, band0 = blockIdx.y * PREP_BAND_ROWS;
  const int band1 = min(band0 + PREP_BAND_ROWS, H);
  const bool white = status != 0 || tile0 >= ow;   // (workgroup-uniform)
  if (!white) {
    if (tile0 + tid < ow) cubic_coef(tile0 + tid, cw, ow, s_x0[tid], s_cx[tid]);
    if (tid < band1 - band0) cubic_coef(band0 + tid, ch, H, s_y0[tid], s_cy[tid]);
    __syncthreads();
  }
  const int d0 = tile0 + 4 * tx;   // W % 4 == 0: the four columns are inside the image together
  if (d0 >= W) return;
  float* out = img_out + (size_t)b * H * W + d0;
  if (white || d0 >= ow) {
    for (int e = band0 + ty; e < band1; e += T / 64) *reinterpret_cast<float4*>(out + (size_t)e * W) = make_float4(255.f, 255.f, 255.f, 255.f);
    return;
  }

  // the four columns' taps, as byte offsets into a source row, and coefficients; a column at or past ow reads the crop's first
  // pixel with zero weights and stores 255
  int off[4][4], cx[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bool in = d0 + c < ow;
    const int x0 = in ? s_x0[4 * tx + c] : 1;
    const int4 k4 = in ? s_cx[4 * tx + c] : make_int4(0, 0, 0, 0);
    cx[c][0] = k4.x, cx[c][1] = k4.y, cx[c][2] = k4.z, cx[c][3] = k4.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) off[c][k] = c0 + (in ? min(max(x0 - 1 + k, 0), cw - 1) : 0);
  }
  // Window path: when no tap of the four columns is clamped (each column's taps are four consecutive bytes) and all sixteen
  // lie in 16 bytes that end inside the crop (downscales up to about 3, and every upscale), a source row costs one 16-byte
  // load; column c's taps are then bytes sh[c]..sh[c]+3 of dwords q[c], q[c]+1 of the window.  Otherwise (the crop's left
  // and right edge, stronger downscales) the sixteen taps are gathered byte by byte.  Same integers either way.
  const int base = off[0][0];
  bool window = d0 + 3 < ow && off[3][3] - base <= 15 && base + 16 <= c0 + cw;
  int q[4], sh[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    window = window && off[c][3] - off[c][0] == 3;
    q[c] = (off[c][0] - base) >> 2;
    sh[c] = (off[c][0] - base) & 3;
  }
  const uint8_t* src = images + (size_t)b * Hin * Win;
  for (int e = band0 + ty; e < band1; e += T / 64) {
    const int y0 = s_y0[e - band0];
    const int4 k4 = s_cy[e - band0];
    const int cy[4] = {k4.x, k4.y, k4.z, k4.w};
    // sum |cx| and sum |cy| are at most 2816 (t = 1/2), so every partial sum is within 255 * 2816^2 = 2 022 113 280 and the
    // rounding term keeps it below 2^31: int32 holds it
    int acc[4] = {0, 0, 0, 0};
    if (window) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* row = src + (size_t)(r0 + min(max(y0 - 1 + j, 0), ch - 1)) * Win;
        uint4 v;
        __builtin_memcpy(&v, row + base, 16);   // (any alignment)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const unsigned lo = q[c] == 0 ? v.x : q[c] == 1 ? v.y : q[c] == 2 ? v.z : v.w;
          const unsigned hi = q[c] == 0 ? v.y : q[c] == 1 ? v.z : v.w;   // (q == 3: sh == 0, hi is not looked at)
          const unsigned p = __builtin_amdgcn_alignbyte(hi, lo, sh[c]);
          const int hs = cx[c][0] * (int)(p & 255u) + cx[c][1] * (int)((p >> 8) & 255u) + cx[c][2] * (int)((p >> 16) & 255u) +
                         cx[c][3] * (int)(p >> 24);
          acc[c] += cy[j] * hs;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* row = src + (size_t)(r0 + min(max(y0 - 1 + j, 0), ch - 1)) * Win;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int hs = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) hs += cx[c][k] * (int)row[off[c][k]];
          acc[c] += cy[j] * hs;
        }
      }
    }
    float val[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = d0 + c < ow ? (float)min(max((acc[c] + (1 << 21)) >> 22, 0), 255) : 255.f;
    *reinterpret_cast<float4*>(out + (size_t)e * W) = make_float4(val[0], val[1], val[2], val[3]);
  }
}

}  // namespace

hipError_t launch_prep(const uint8_t* images, const int32_t* sizes, int B, int Hin, int Win, int H, int W, int thresh, float* img_out,
                       int32_t* widths_out, int32_t* boxes_out, int32_t* status_out, int32_t* boxes, hipStream_t st) {
  hipLaunchKernelGGL(prep_init_kernel, dim3((B + T - 1) / T), dim3(T), 0, st, boxes, B);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 box_grid((Win + PREP_BOX_COLS - 1) / PREP_BOX_COLS, (Hin + PREP_BOX_ROWS - 1) / PREP_BOX_ROWS, B);
  hipLaunchKernelGGL(prep_box_kernel, box_grid, dim3(T), 0, st, images, sizes, Hin, Win, thresh, boxes);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 resize_grid((W + PREP_TILE_COLS - 1) / PREP_TILE_COLS, (H + PREP_BAND_ROWS - 1) / PREP_BAND_ROWS, B);
  hipLaunchKernelGGL(prep_resize_kernel, resize_grid, dim3(T), 0, st, images, sizes, Hin, Win, H, W, boxes, img_out, widths_out, boxes_out,
                     status_out);
  return hipGetLastError();
}
