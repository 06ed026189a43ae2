// encode.hip — the stroke encoder (include/dhw.h: dhw_encode): raw pen points [B,N,3] = (x, y, end) -> the
// model's strokes [B,L,3] = (dx, dy, pen), normalised and thinned as the training corpus was.  One kernel, one workgroup per
// line, the line resident in LDS as fp64 offsets plus a pen byte:
//   load       offsets of consecutive points (y negated), the end flags rolled by one into the pen column
//   normalise  two-pass population std of all dx and dy as one set, summed in a fixed tree; divide
//   round      keys v_j of the pairs (2j, 2j+1); pair j merges iff fewer than k pairs come before it in (v, j) order (a rank by
//              counting: every thread walks all keys through LDS broadcasts); ballot prefix scan of the merge flags;
//              compaction in place through registers; normalise again
//   store      f32 roundings, (0, 0, 1) padding, length and status
// Row i (pair j) belongs to thread i % 256 (j % 256) whatever N, L or B are, every sum is a fixed tree over those threads, no
// atomics are used and floating-point contraction is off: a line gives the same bits alone, in any batch, in either instance.
#include "encode.h"

#pragma clang fp contract(off)

namespace {

constexpr int T = ENCODE_THREADS;
constexpr int WAVES = T / 64;

// all-lanes sum / max over the workgroup in a fixed tree: xor butterfly inside a wave (a + b on both partners: the same bits
// in every lane), then the four wave values as (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double block_sum(double v, double* s_red, int lane, int wave) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();   // the previous reduction's readers are done with s_red
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
__device__ __forceinline__ double block_max(double v, double* s_red, int lane, int wave) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  return fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}

// rule 3: divide the M rows by the population std of their 2M values; false (nothing divided) when the std is 0 or not finite.
// The result is the same in every thread.  Ends with a barrier.
__device__ __forceinline__ bool normalise(double* s_x, double* s_y, int M, double* s_red, int tid, int lane, int wave) {
  const double cnt = 2.0 * (double)M;
  double sum = 0.0;
  for (int i = tid; i < M; i += T) {
    sum += s_x[i];
    sum += s_y[i];
  }
  const double mean = block_sum(sum, s_red, lane, wave) / cnt;
  double sq = 0.0;
  for (int i = tid; i < M; i += T) {
    const double ex = s_x[i] - mean, ey = s_y[i] - mean;
    sq += ex * ex;
    sq += ey * ey;
  }
  const double sd = sqrt(block_sum(sq, s_red, lane, wave) / cnt);
  if (!(sd > 0.0) || !isfinite(sd)) return false;
  for (int i = tid; i < M; i += T) {
    s_x[i] /= sd;
    s_y[i] /= sd;
  }
  __syncthreads();
  return true;
}

template <int MAXN>
__global__ __launch_bounds__(T) void encode_kernel(const float* __restrict__ points, const int32_t* __restrict__ counts, int N, int L,
                                                   int rounds, float max_abs, float* __restrict__ strokes_out,
                                                   int32_t* __restrict__ lens_out, int32_t* __restrict__ status_out) {
  constexpr int PAIRS = MAXN / 2;
  constexpr int SLOTS = PAIRS / T;   // pairs per thread: pair j sits in slot j / 256 of thread j % 256
  __shared__ double s_x[MAXN];
  __shared__ double s_y[MAXN];
  __shared__ double s_v[PAIRS];
  __shared__ unsigned char s_pen[MAXN];
  __shared__ double s_red[WAVES];
  __shared__ int s_cnt[SLOTS][WAVES];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* out = strokes_out + (size_t)b * L * 3;
  const int n = counts ? counts[b] : N;
  if (n < 2 || n > N) {   // rule 6 bit 1 (workgroup-uniform): nothing of the line is read
    for (int q = tid; q < 3 * L; q += T) out[q] = (q % 3 == 2) ? 1.f : 0.f;
    if (tid == 0) {
      lens_out[b] = 0;
      status_out[b] = 1;
    }
    return;
  }

  // rules 1 and 2.  Point i + 1 is the last one read: nothing at or past n.
  const float* src = points + (size_t)b * N * 3;
  int M = n - 1;
  int bad = 0;
  for (int i = tid; i < M; i += T) {
    const float* p = src + 3 * i;
    const float x0 = p[0], y0 = p[1], x1 = p[3], y1 = p[4], e1 = p[5];
    bad |= !isfinite(x1) || !isfinite(y1) || !isfinite(e1);
    if (i == 0) bad |= !isfinite(x0) || !isfinite(y0) || !isfinite(p[2]);
    s_x[i] = (double)x1 - (double)x0;
    s_y[i] = -((double)y1 - (double)y0);
    s_pen[i + 1 == M ? 0 : i + 1] = e1 != 0.f;
  }
  bad = __syncthreads_or(bad);   // (also the barrier between the fill and its readers)
  if (!bad) bad = !normalise(s_x, s_y, M, s_red, tid, lane, wave);

  // rule 4.  Once bit 2 is known the values mean nothing: only the row count goes on shrinking.
  for (int r = 0; r < rounds; ++r) {
    const int k = M / 5, P = M / 2;
    if (bad) {
      M -= k;
      continue;
    }
    double v[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int j = s * T + tid;
      v[s] = 0.0;
      if (j < P) {
        const double ax = s_x[2 * j], ay = s_y[2 * j], bx = s_x[2 * j + 1], by = s_y[2 * j + 1];
        const double cx = ax + bx, cy = ay + by;
        v[s] = sqrt(ax * ax + ay * ay) + sqrt(bx * bx + by * by) - sqrt(cx * cx + cy * cy);
        s_v[j] = v[s];
      }
    }
    __syncthreads();

    // before[s] = the pairs that come before pair j in (v, j) order; every lane reads the same key: an LDS broadcast
    int before[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) before[s] = 0;
    for (int q = 0; q < P; ++q) {
      const double w = s_v[q];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (s * T < P) before[s] += (w < v[s] || (w == v[s] && q < s * T + tid)) ? 1 : 0;
    }

    // merge flags -> exclusive prefix in pair order (slot-major, then wave, then lane); the rows go through registers so
    // that the compaction can run in place
    double x0[SLOTS], y0[SLOTS], x1[SLOTS], y1[SLOTS];
    unsigned pen0 = 0, pen1 = 0, merged = 0;
    int pre[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int j = s * T + tid;
      const bool m = j < P && before[s] < k;
      x0[s] = y0[s] = x1[s] = y1[s] = 0.0;
      if (j < P) {
        x0[s] = s_x[2 * j];
        y0[s] = s_y[2 * j];
        x1[s] = s_x[2 * j + 1];
        y1[s] = s_y[2 * j + 1];
        pen0 |= (unsigned)s_pen[2 * j] << s;
        pen1 |= (unsigned)s_pen[2 * j + 1] << s;
      }
      merged |= (unsigned)m << s;
      const unsigned long long vote = __ballot(m);
      pre[s] = __popcll(vote & ((1ull << lane) - 1ull));
      if (lane == 0) s_cnt[s][wave] = __popcll(vote);
    }
    // an odd last row has no partner: it only moves
    const bool tail = (M & 1) && tid == 0;
    double tx = 0.0, ty = 0.0;
    unsigned char tp = 0;
    if (tail) {
      tx = s_x[M - 1];
      ty = s_y[M - 1];
      tp = s_pen[M - 1];
    }
    __syncthreads();   // every row is in a register, every count is in LDS
    int base = 0;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      int mine = base + pre[s];
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w < wave) mine += s_cnt[s][w];
        base += s_cnt[s][w];
      }
      const int j = s * T + tid;
      if (j < P) {
        const int d = 2 * j - mine;   // <= 2j: `mine` merged pairs before j deleted one row each
        const unsigned p0 = (pen0 >> s) & 1u, p1 = (pen1 >> s) & 1u;
        if ((merged >> s) & 1u) {
          s_x[d] = x0[s] + x1[s];
          s_y[d] = y0[s] + y1[s];
          s_pen[d] = (unsigned char)(p0 | p1);
        } else {
          s_x[d] = x0[s];
          s_y[d] = y0[s];
          s_pen[d] = (unsigned char)p0;
          s_x[d + 1] = x1[s];
          s_y[d + 1] = y1[s];
          s_pen[d + 1] = (unsigned char)p1;
        }
      }
    }
    if (tail) {   // base == k here: exactly k pairs have fewer than k pairs before them
      s_x[M - 1 - k] = tx;
      s_y[M - 1 - k] = ty;
      s_pen[M - 1 - k] = tp;
    }
    M -= k;
    __syncthreads();
    bad = !normalise(s_x, s_y, M, s_red, tid, lane, wave);
  }

  int status = bad ? 2 : 0;
  if (M > L) status |= 4;
  if (!bad) {
    double big = 0.0;
    for (int i = tid; i < M; i += T) big = fmax(big, fmax(fabs(s_x[i]), fabs(s_y[i])));
    if (block_max(big, s_red, lane, wave) > (double)max_abs) status |= 8;
  }
  // rules 7 and 8 (status is workgroup-uniform; with status 0, M <= L)
  for (int q = tid; q < 3 * L; q += T) {
    const int i = q / 3, c = q - 3 * i;
    float val = (c == 2) ? 1.f : 0.f;
    if (status == 0 && i < M) val = c == 0 ? (float)s_x[i] : c == 1 ? (float)s_y[i] : (float)s_pen[i];
    out[q] = val;
  }
  if (tid == 0) {
    lens_out[b] = M;
    status_out[b] = status;
  }
}

}  // namespace

hipError_t launch_encode(const float* points, const int32_t* counts, int B, int N, int L, int rounds, float max_abs,
                         float* strokes_out, int32_t* lens_out, int32_t* status_out, hipStream_t st) {
  if (N <= ENCODE_SMALL_N)
    hipLaunchKernelGGL(encode_kernel<ENCODE_SMALL_N>, dim3(B), dim3(T), 0, st, points, counts, N, L, rounds, max_abs, strokes_out, lens_out,
                       status_out);
  else
    hipLaunchKernelGGL(encode_kernel<ENCODE_MAX_N>, dim3(B), dim3(T), 0, st, points, counts, N, L, rounds, max_abs, strokes_out, lens_out,
                       status_out);
  return hipGetLastError();
}
