// moments.hip — first and second moments of pooled feature vectors in double precision (include/dhw.h dhw_moments_update;
// DESIGN.md §37).  Three launches on one stream:
//   moments_pool_kernel   p[n][d] = (sum_s (double)feat[n][s][d]) / S, s ascending, into the workspace (f64 [N,D])
//   moments_sum_kernel    sum[d] += sum_n p[n][d]: 16 strided partial sums per column, joined in a fixed order
//   moments_gram_kernel   gram += p^T p on v_mfma_f64_16x16x4_f64, one owning workgroup per 64 x 64 block with I <= J
// No atomics anywhere: the same call on the same state gives the same bits.
#include "moments.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(MOMENTS_THREADS) void moments_pool_kernel(const float* __restrict__ feat, int N, int S, int D,
                                                                      double* __restrict__ p) {
  const size_t idx = (size_t)blockIdx.x * MOMENTS_THREADS + threadIdx.x;
  if (idx >= (size_t)N * D) return;
  const size_t n = idx / D, d = idx - n * D;
  const float* f = feat + n * S * D + d;
  double acc = (double)f[0];
  for (int s = 1; s < S; ++s) acc += (double)f[(size_t)s * D];
  p[idx] = acc / (double)S;
}

// One workgroup per 16 columns: thread (r, c) adds rows n = r, r + 16, ... of column c in ascending order, thread (0, c) joins
// the 16 partial sums in the order r = 0 .. 15 and adds the total to sum.
__global__ __launch_bounds__(MOMENTS_THREADS) void moments_sum_kernel(const double* __restrict__ p, int N, int D, double* __restrict__ sum) {
  __shared__ double part[16][16];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int d = blockIdx.x * 16 + c;   // D is a multiple of 16: always a column
  double acc = 0.0;
  int n = r;
  for (; n + 16 * 7 < N; n += 16 * 8) {   // eight loads in flight, added in the same ascending order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(n + 16 * u) * D + d];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; n < N; n += 16) acc += p[(size_t)n * D + d];
  part[r][c] = acc;
  __syncthreads();
  if (r == 0) {
    double total = part[0][c];
    for (int q = 1; q < 16; ++q) total += part[q][c];
    sum[d] += total;
  }
}

// The walk over n of one wave's 2 x 2 tiles.  Operands: A[i = lane & 15][k = lane >> 4] = p[n0 + k][i0 + i] and
// B[k = lane >> 4][j = lane & 15] = p[n0 + k][j0 + j], one double per lane, both read straight from the k-major pooled matrix
// (16 consecutive doubles per k row).  mask bit 2 m + q: tile (m, q) is wanted; ALL: every tile is.  Rows go through the matrix
// pipe in ascending order, four per instruction; the operands of the next 16 rows are requested before the 16 instructions of
// the current ones issue.
struct GramOperands {
  double a0[4], a1[4], b0[4], b1[4];   // [u]: the K group of rows n0 + 4 u .. n0 + 4 u + 3
};

template <bool ALL>
__device__ __forceinline__ void gram_step(double a0, double a1, double b0, double b1, int mask, f64x4 (&acc)[2][2]) {
  if (ALL || (mask & 1)) acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
  if (ALL || (mask & 2)) acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
  if (ALL || (mask & 4)) acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
  if (ALL || (mask & 8)) acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
}

__device__ __forceinline__ void gram_load(GramOperands& g, const double* pa0, const double* pa1, const double* pb0, const double* pb1, int n0,
                                          int D) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const size_t o = (size_t)(n0 + 4 * u) * D;
    g.a0[u] = pa0[o];
    g.a1[u] = pa1[o];
    g.b0[u] = pb0[o];
    g.b1[u] = pb1[o];
  }
}

template <bool ALL>
__device__ __forceinline__ void gram_walk(const double* __restrict__ pa0, const double* __restrict__ pa1, const double* __restrict__ pb0,
                                          const double* __restrict__ pb1, int N, int D, int k, int mask, f64x4 (&acc)[2][2]) {
  const int full = N & ~3;
  int n0 = 0;
  if (full >= 16) {
    GramOperands cur, nxt;
    gram_load(cur, pa0, pa1, pb0, pb1, 0, D);
    for (; n0 + 16 <= full; n0 += 16) {
      const bool more = n0 + 32 <= full;
      if (more) gram_load(nxt, pa0, pa1, pb0, pb1, n0 + 16, D);
#pragma unroll
      for (int u = 0; u < 4; ++u) gram_step<ALL>(cur.a0[u], cur.a1[u], cur.b0[u], cur.b1[u], mask, acc);
      if (more) cur = nxt;
    }
  }
  for (; n0 < full; n0 += 4) {
    const size_t o = (size_t)n0 * D;
    gram_step<ALL>(pa0[o], pa1[o], pb0[o], pb1[o], mask, acc);
  }
  if (full < N) {   // the last N % 4 rows: rows at or past N are literal zeros, the memory behind row N is never read
    const size_t o = (size_t)full * D;
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    if (full + k < N) { a0 = pa0[o]; a1 = pa1[o]; b0 = pb0[o]; b1 = pb1[o]; }
    gram_step<ALL>(a0, a1, b0, b1, mask, acc);
  }
}

// Workgroup b owns block (I, J), I <= J, of the upper triangle of ceil(D / 64)^2 blocks, and its mirror (J, I).  Wave w holds
// tiles (2 (w >> 1) + m, 2 (w & 1) + q) of the block's 4 x 4.  A tile is computed iff it lies inside D and its row offset is
// not below its column offset (i0 <= j0): in a diagonal block the tiles under the diagonal are the mirrors of those above.
// The owner reads the tile's current value as the accumulator, walks n ascending and writes it back with its mirror; of a
// diagonal tile only the elements with row <= col are written (and mirrored), so gram is bitwise symmetric whatever the
// matrix pipe does with a swapped operand pair.  C/D map of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg.
__global__ __launch_bounds__(MOMENTS_THREADS) void moments_gram_kernel(const double* __restrict__ p, int N, int D, double* __restrict__ gram) {
  const int nb = (D + MOMENTS_BLOCK - 1) / MOMENTS_BLOCK;
  int b = blockIdx.x, I = 0;
  while (b >= nb - I) { b -= nb - I; ++I; }
  const int J = I + b;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int c = lane & 15, k = lane >> 4;
  int i0[2], j0[2], mask = 0;
  for (int m = 0; m < 2; ++m) {
    i0[m] = I * MOMENTS_BLOCK + (wave >> 1) * 32 + m * 16;
    j0[m] = J * MOMENTS_BLOCK + (wave & 1) * 32 + m * 16;
  }
  for (int m = 0; m < 2; ++m)
    for (int q = 0; q < 2; ++q)
      if (i0[m] < D && j0[q] < D && i0[m] <= j0[q]) mask |= 1 << (2 * m + q);
  if (!mask) return;

  f64x4 acc[2][2];
  for (int m = 0; m < 2; ++m)
    for (int q = 0; q < 2; ++q)
      for (int r = 0; r < 4; ++r)
        acc[m][q][r] = (mask >> (2 * m + q) & 1) ? gram[(size_t)(i0[m] + k + 4 * r) * D + j0[q] + c] : 0.0;

  // a tile row / column outside D is never wanted: its operand reads column 0 instead, in bounds, and the product is not kept
  const double* row = p + (size_t)k * D + c;
  const double *pa0 = row + (i0[0] < D ? i0[0] : 0), *pa1 = row + (i0[1] < D ? i0[1] : 0);
  const double *pb0 = row + (j0[0] < D ? j0[0] : 0), *pb1 = row + (j0[1] < D ? j0[1] : 0);
  if (mask == 15)
    gram_walk<true>(pa0, pa1, pb0, pb1, N, D, k, mask, acc);
  else
    gram_walk<false>(pa0, pa1, pb0, pb1, N, D, k, mask, acc);

  for (int m = 0; m < 2; ++m)
    for (int q = 0; q < 2; ++q) {
      if (!(mask >> (2 * m + q) & 1)) continue;
      const bool diag = i0[m] == j0[q];
      for (int r = 0; r < 4; ++r) {
        const int gi = i0[m] + k + 4 * r, gj = j0[q] + c;
        const double v = acc[m][q][r];
        if (!diag || gi <= gj) gram[(size_t)gi * D + gj] = v;
        if (!diag || gi < gj) gram[(size_t)gj * D + gi] = v;
      }
    }
}

hipError_t launch_moments_pool(const float* feat, int N, int S, int D, double* pooled, hipStream_t st) {
  const size_t cells = (size_t)N * D;
  hipLaunchKernelGGL(moments_pool_kernel, dim3((unsigned)((cells + MOMENTS_THREADS - 1) / MOMENTS_THREADS)), dim3(MOMENTS_THREADS), 0, st, feat, N, S, D, pooled);
  return hipGetLastError();
}

hipError_t launch_moments(const float* feat, int N, int S, int D, double* sum, double* gram, double* pooled, hipStream_t st) {
  const int nb = (D + MOMENTS_BLOCK - 1) / MOMENTS_BLOCK;
  const hipError_t e = launch_moments_pool(feat, N, S, D, pooled, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(moments_sum_kernel, dim3(D / 16), dim3(MOMENTS_THREADS), 0, st, pooled, N, D, sum);
  hipLaunchKernelGGL(moments_gram_kernel, dim3(nb * (nb + 1) / 2), dim3(MOMENTS_THREADS), 0, st, pooled, N, D, gram);
  return hipGetLastError();
}
