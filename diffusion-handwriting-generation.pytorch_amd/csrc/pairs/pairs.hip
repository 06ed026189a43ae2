// pairs.hip — pairwise statistics of two sets of f64 feature vectors (include/dhw.h dhw_pairs_knn / _cover / _polysum; DESIGN.md
// §38).  The M x N matrix of inner products is computed on v_mfma_f64_16x16x4_f64 and reduced in the epilogue; it is never written.
//   pairs_transpose_kernel   x [N][D] -> xt [D][Np], k-major, zeros in the columns at or past N (Np = N rounded up to 64)
//   pairs_sq_kernel          sq[n] = sum_d x[n][d]^2, one wave per row, zero at or past N
//   pairs_kernel<MODE>       workgroup (row block, split): 64 rows against the split's share of the 64-column chunks
//   pairs_*_merge_kernel     the splits' partial results joined in a fixed order
// No atomics, one writer per output element, rows at or past M / N never read: the same call gives the same bits.
#include "pairs.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { PAIRS_KNN = 0, PAIRS_COVER = 1, PAIRS_POLY = 2 };

constexpr int PAIRS_LDS_STRIDE = PAIRS_BLOCK + 1;   // the staged d2 tile: 64 rows of 65 doubles

__global__ __launch_bounds__(PAIRS_THREADS) void pairs_transpose_kernel(const double* __restrict__ x, int N, int D, int Np, double* __restrict__ xt) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8 threads, a 32 x 32 tile
  const int n0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 8 * i, d = d0 + tx;
    tile[ty + 8 * i][tx] = (n < N && d < D) ? x[(size_t)n * D + d] : 0.0;
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int d = d0 + ty + 8 * i;
    if (d < D) xt[(size_t)d * Np + n0 + tx] = tile[tx][ty + 8 * i];   // n0 + tx < Np: the grid covers Np / 32 tiles
  }
}

// One wave per row: lane l adds d = l, l + 64, ... ascending, the 64 partial sums are joined by a fixed butterfly.
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_sq_kernel(const double* __restrict__ x, int N, int D, int Np, double* __restrict__ sq) {
  const int n = blockIdx.x * (PAIRS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= Np) return;
  double acc = 0.0;
  if (n < N)
    for (int d = lane; d < D; d += 64) {
      const double v = x[(size_t)n * D + d];
      acc = fma(v, v, acc);
    }
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) sq[n] = acc;
}

struct PairsArgs {
  const double *xt, *yt, *sqx, *sqy;   // k-major operands [D][Mp] / [D][Np] and the squared norms
  int M, N, D, Mp, Np, splits;
  const double* radius2;               // PAIRS_COVER: [N] or NULL
  int skip_diag;                       // PAIRS_POLY
  double* part;                        // the partial results (pairs.h)
};

// The operands of 16 consecutive d of one wave's 2 x 2 tiles: A[i = lane & 15][k = lane >> 4] = xt[d0 + k][i0 + i] and
// B[k][j = lane & 15] = yt[d0 + k][j0 + j], one double per lane, 16 consecutive doubles per k row (the layout of
// moments_gram_kernel).  [t][u]: tile t, the K group d0 + 4 u .. d0 + 4 u + 3.
struct PairsOperands {
  double a[2][4], b[2][4];
};

__device__ __forceinline__ void pairs_load(PairsOperands& g, const double* pa, const double* pb, size_t sa, size_t sb) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    g.a[0][u] = pa[4 * u * sa];
    g.a[1][u] = pa[4 * u * sa + 16];
    g.b[0][u] = pb[4 * u * sb];
    g.b[1][u] = pb[4 * u * sb + 16];
  }
}

// acc[m][q] = the 16 x 16 tile of inner products of rows i0 + 16 m .. and columns j0 + 16 q .., d ascending, four d per
// instruction; the operands of the next 16 d are requested before the 16 instructions of the current ones issue.  D is a
// multiple of 16 and the padded columns are zeros, so there is no tail and no read outside xt / yt.
__device__ __forceinline__ void pairs_dots(const double* __restrict__ pa, const double* __restrict__ pb, int D, size_t sa, size_t sb, f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[m][q] = f64x4{0.0, 0.0, 0.0, 0.0};
  PairsOperands cur, nxt;
  pairs_load(cur, pa, pb, sa, sb);
  for (int d0 = 0; d0 < D; d0 += 16) {
    const bool more = d0 + 16 < D;
    if (more) pairs_load(nxt, pa + (size_t)(d0 + 16) * sa, pb + (size_t)(d0 + 16) * sb, sa, sb);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.a[m][u], cur.b[q][u], acc[m][q], 0, 0, 0);
    if (more) cur = nxt;
  }
}

// keep the PAIRS_MAX_K smallest values seen, ascending (static indices only: the list stays in registers)
__device__ __forceinline__ void pairs_insert(double (&best)[PAIRS_MAX_K], double v) {
  if (v < best[PAIRS_MAX_K - 1]) {
    best[PAIRS_MAX_K - 1] = v;
#pragma unroll
    for (int i = PAIRS_MAX_K - 1; i > 0; --i)
      if (best[i] < best[i - 1]) {
        const double t = best[i];
        best[i] = best[i - 1];
        best[i - 1] = t;
      }
  }
}

// Workgroup (b, s): rows 64 b .. 64 b + 63 against the 64-column chunks [s nc / S, (s + 1) nc / S) of nc = Np / 64.  Wave w holds
// the 2 x 2 tiles at rows 32 (w >> 1), columns 32 (w & 1) of each 64 x 64 chunk.  C/D map of the f64 form: col = lane & 15,
// row = (lane >> 4) + 4 reg, so a lane holds 8 rows x 2 columns of a chunk.  d2 = fmax(0, sq_i + sq_j - 2 dot).
//   PAIRS_KNN    the chunk's d2 go through LDS (+inf for j == i and j >= N); thread t keeps the 8 smallest of row t >> 2 in the
//                columns 16 (t & 3) ..; at the end the four lists of a row are merged and written as the split's 8 candidates
//   PAIRS_COVER  per lane and row: count of d2 <= radius2[j], min and smallest argmin, in registers; joined over the 32 lanes
//                of a row through LDS (ties: the smaller index)
//   PAIRS_POLY   per lane: sum of (dot + D)^3 in a fixed order; the 256 sums are added in thread order
template <int MODE>
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_kernel(PairsArgs p) {
  __shared__ double lds[PAIRS_BLOCK * PAIRS_LDS_STRIDE];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, t = threadIdx.x;
  const int c = lane & 15, kq = lane >> 4;
  const int rb = blockIdx.x, split = blockIdx.y;
  const int nc = p.Np / PAIRS_BLOCK;
  const int ch_lo = (int)((long long)split * nc / p.splits), ch_hi = (int)((long long)(split + 1) * nc / p.splits);
  const int li = (wave >> 1) * 32, lj = (wave & 1) * 32;
  const int i0 = rb * PAIRS_BLOCK + li;
  const size_t sa = (size_t)p.Mp, sb = (size_t)p.Np;
  const double* pa = p.xt + (size_t)kq * sa + i0 + c;

  double sx[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) sx[m][r] = p.sqx[i0 + 16 * m + kq + 4 * r];

  const double inf = __builtin_huge_val();
  double best[PAIRS_MAX_K];          // PAIRS_KNN
  double mn[2][4];                   // PAIRS_COVER
  int mi[2][4], cnt[2][4];
  double total = 0.0;                // PAIRS_POLY
#pragma unroll
  for (int i = 0; i < PAIRS_MAX_K; ++i) best[i] = inf;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) { mn[m][r] = inf; mi[m][r] = 0x7fffffff; cnt[m][r] = 0; }

  for (int ch = ch_lo; ch < ch_hi; ++ch) {
    const int j0 = ch * PAIRS_BLOCK + lj;
    f64x4 acc[2][2];
    pairs_dots(pa, p.yt + (size_t)kq * sb + j0 + c, p.D, sa, sb, acc);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int col = j0 + 16 * q + c;
      const bool in = col < p.N;
      const double sy = p.sqy[col];   // col < Np
      double rad = -1.0;              // no d2 is <= -1: nothing is counted without a radius or past N
      if (MODE == PAIRS_COVER && p.radius2 && in) rad = p.radius2[col];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lrow = li + 16 * m + kq + 4 * r, row = rb * PAIRS_BLOCK + lrow;
          const double dot = acc[m][q][r];
          if (MODE == PAIRS_POLY) {
            const double v = dot + (double)p.D;
            if (in && row < p.M && !(p.skip_diag && row == col)) total += v * v * v;
          } else {
            const double d2 = fmax(0.0, sx[m][r] + sy - 2.0 * dot);
            if (MODE == PAIRS_KNN) {
              lds[lrow * PAIRS_LDS_STRIDE + lj + 16 * q + c] = (in && row != col) ? d2 : inf;
            } else if (in) {
              cnt[m][r] += d2 <= rad;
              if (d2 < mn[m][r]) { mn[m][r] = d2; mi[m][r] = col; }
            }
          }
        }
    }
    if (MODE == PAIRS_KNN) {
      __syncthreads();
      const double* mine = lds + (t >> 2) * PAIRS_LDS_STRIDE + (t & 3) * 16;
      for (int cc = 0; cc < 16; ++cc) pairs_insert(best, mine[cc]);
      __syncthreads();
    }
  }

  if (MODE == PAIRS_KNN) {
#pragma unroll
    for (int i = 0; i < PAIRS_MAX_K; ++i) lds[t * PAIRS_MAX_K + i] = best[i];   // row t >> 2, list t & 3
    __syncthreads();
    if (t < PAIRS_BLOCK) {
      double all[PAIRS_MAX_K];
#pragma unroll
      for (int i = 0; i < PAIRS_MAX_K; ++i) all[i] = inf;
      for (int i = 0; i < 4 * PAIRS_MAX_K; ++i) pairs_insert(all, lds[t * 4 * PAIRS_MAX_K + i]);
      double* out = p.part + ((size_t)split * p.Mp + rb * PAIRS_BLOCK + t) * PAIRS_MAX_K;
#pragma unroll
      for (int i = 0; i < PAIRS_MAX_K; ++i) out[i] = all[i];
    }
  } else if (MODE == PAIRS_COVER) {
    double* lmn = lds;                                   // [64][32]
    int* lmi = (int*)(lds + PAIRS_BLOCK * 32);           // [64][32]
    int* lcnt = lmi + PAIRS_BLOCK * 32;                  // [64][32]: 16 + 8 + 8 KiB of the 32.5 KiB
    const int slot = (wave & 1) * 16 + c;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = (li + 16 * m + kq + 4 * r) * 32 + slot;
        lmn[o] = mn[m][r];
        lmi[o] = mi[m][r];
        lcnt[o] = cnt[m][r];
      }
    __syncthreads();
    if (t < PAIRS_BLOCK) {
      double bm = inf;
      int bi = 0x7fffffff, n = 0;
      for (int s = 0; s < 32; ++s) {
        const double v = lmn[t * 32 + s];
        const int j = lmi[t * 32 + s];
        n += lcnt[t * 32 + s];
        if (v < bm || (v == bm && j < bi)) { bm = v; bi = j; }
      }
      const size_t o = (size_t)split * p.Mp + rb * PAIRS_BLOCK + t;
      int* pint = (int*)(p.part + (size_t)p.splits * p.Mp);
      p.part[o] = bm;
      pint[2 * o] = n;
      pint[2 * o + 1] = bi;
    }
  } else {
    lds[t] = total;
    __syncthreads();
    if (t == 0) {
      double s = lds[0];
      for (int i = 1; i < PAIRS_THREADS; ++i) s += lds[i];
      p.part[(size_t)rb * p.splits + split] = s;
    }
  }
}

// radius2[i] = the k-th smallest of the splits' candidates of row i (a multiset's order statistic: no order dependence)
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_knn_merge_kernel(const double* __restrict__ part, int N, int Mp, int splits, int k,
                                                                         double* __restrict__ radius2) {
  const int row = blockIdx.x * PAIRS_THREADS + threadIdx.x;
  if (row >= N) return;
  double best[PAIRS_MAX_K];
#pragma unroll
  for (int i = 0; i < PAIRS_MAX_K; ++i) best[i] = __builtin_huge_val();
  for (int s = 0; s < splits; ++s) {
    const double* in = part + ((size_t)s * Mp + row) * PAIRS_MAX_K;
    for (int i = 0; i < PAIRS_MAX_K; ++i) pairs_insert(best, in[i]);
  }
  double out = best[0];
#pragma unroll
  for (int i = 1; i < PAIRS_MAX_K; ++i)
    if (i == k - 1) out = best[i];
  radius2[row] = out;
}

// splits ascending: the counts add, the minimum keeps the smaller index on a tie
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_cover_merge_kernel(const double* __restrict__ part, int M, int Mp, int splits, int* __restrict__ count,
                                                                           double* __restrict__ nearest2, int* __restrict__ nearest_idx) {
  const int row = blockIdx.x * PAIRS_THREADS + threadIdx.x;
  if (row >= M) return;
  const int* pint = (const int*)(part + (size_t)splits * Mp);
  double bm = __builtin_huge_val();
  int bi = 0x7fffffff, n = 0;
  for (int s = 0; s < splits; ++s) {
    const size_t o = (size_t)s * Mp + row;
    const double v = part[o];
    const int j = pint[2 * o + 1];
    n += pint[2 * o];
    if (v < bm || (v == bm && j < bi)) { bm = v; bi = j; }
  }
  if (count) count[row] = n;
  nearest2[row] = bm;
  if (nearest_idx) nearest_idx[row] = bi;
}

// one workgroup: thread t adds the partial sums t, t + 256, ... ascending, thread 0 adds the 256 results in thread order
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_poly_merge_kernel(const double* __restrict__ part, int count, double* __restrict__ out) {
  __shared__ double red[PAIRS_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += PAIRS_THREADS) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = red[0];
    for (int i = 1; i < PAIRS_THREADS; ++i) total += red[i];
    out[0] = total;
  }
}

// x [N][D] -> its k-major copy and squared norms in the workspace
static void pairs_prepare(const double* x, int N, int D, int Np, double* xt, double* sq, hipStream_t st) {
  hipLaunchKernelGGL(pairs_transpose_kernel, dim3(Np / 32, (D + 31) / 32), dim3(PAIRS_THREADS), 0, st, x, N, D, Np, xt);
  hipLaunchKernelGGL(pairs_sq_kernel, dim3(Np / (PAIRS_THREADS / 64)), dim3(PAIRS_THREADS), 0, st, x, N, D, Np, sq);
}

// both sets prepared (one when they are the same rows) and the kernel's arguments filled
static PairsArgs pairs_setup(const double* x, int M, const double* y, int N, int D, double* ws, int splits, hipStream_t st) {
  const PairsLayout l = pairs_layout(M, N, D);
  PairsArgs a = {};
  pairs_prepare(x, M, D, l.Mp, ws + l.xt, ws + l.sqx, st);
  const bool same = x == y && M == N;
  if (!same) pairs_prepare(y, N, D, l.Np, ws + l.yt, ws + l.sqy, st);
  a.xt = ws + l.xt;
  a.sqx = ws + l.sqx;
  a.yt = same ? a.xt : ws + l.yt;
  a.sqy = same ? a.sqx : ws + l.sqy;
  a.M = M; a.N = N; a.D = D; a.Mp = l.Mp; a.Np = l.Np; a.splits = splits;
  a.part = ws + l.part;
  return a;
}

hipError_t launch_pairs_knn(const double* x, int N, int D, int k, double* radius2, double* ws, int splits, hipStream_t st) {
  PairsArgs a = pairs_setup(x, N, x, N, D, ws, splits, st);
  hipLaunchKernelGGL(pairs_kernel<PAIRS_KNN>, dim3(a.Mp / PAIRS_BLOCK, splits), dim3(PAIRS_THREADS), 0, st, a);
  hipLaunchKernelGGL(pairs_knn_merge_kernel, dim3((N + PAIRS_THREADS - 1) / PAIRS_THREADS), dim3(PAIRS_THREADS), 0, st, a.part, N, a.Mp, splits, k, radius2);
  return hipGetLastError();
}

hipError_t launch_pairs_cover(const double* q, int M, const double* ref, int N, int D, const double* radius2, int* count, double* nearest2,
                              int* nearest_idx, double* ws, int splits, hipStream_t st) {
  PairsArgs a = pairs_setup(q, M, ref, N, D, ws, splits, st);
  a.radius2 = radius2;
  hipLaunchKernelGGL(pairs_kernel<PAIRS_COVER>, dim3(a.Mp / PAIRS_BLOCK, splits), dim3(PAIRS_THREADS), 0, st, a);
  hipLaunchKernelGGL(pairs_cover_merge_kernel, dim3((M + PAIRS_THREADS - 1) / PAIRS_THREADS), dim3(PAIRS_THREADS), 0, st, a.part, M, a.Mp, splits, count,
                     nearest2, nearest_idx);
  return hipGetLastError();
}

hipError_t launch_pairs_polysum(const double* x, int M, const double* y, int N, int D, int skip_diag, double* out, double* ws, int splits,
                                hipStream_t st) {
  PairsArgs a = pairs_setup(x, M, y, N, D, ws, splits, st);
  a.skip_diag = skip_diag;
  hipLaunchKernelGGL(pairs_kernel<PAIRS_POLY>, dim3(a.Mp / PAIRS_BLOCK, splits), dim3(PAIRS_THREADS), 0, st, a);
  hipLaunchKernelGGL(pairs_poly_merge_kernel, dim3(1), dim3(PAIRS_THREADS), 0, st, a.part, a.Mp / PAIRS_BLOCK * splits, out);
  return hipGetLastError();
}
