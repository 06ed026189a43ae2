// dtw.hip — dynamic time warping between every line of a set a and every line of a set b (include/dhw.h dhw_dtw).
//   dtw_kernel<C, F, WITH_K>   one wave per (reference line q, run of consecutive queries): a wavefront recurrence in registers
//   dtw_nearest_kernel         one wave per query: the smallest entry of its row of the [M,N] matrix and the smallest q attaining it
// The recurrence is serial along both axes, so a wave works on one anti-diagonal at a time: lane l owns the C columns
// l C .. l C + C - 1 of the reference (their features, D and K in registers, indexed statically) and at step t works on the
// query row t - l.  What a lane needs from its left neighbour, the D and K of that neighbour's last column one step ago, and the
// query row itself move one lane to the right per step with a DPP move (wave_shr:1); lane 0 takes the new row instead.
// The queries of a run follow one another without a gap: the row that opens a query carries a flag that resets the boundary,
// the row that closes it makes the lane owning column m - 1 write the pair's result.  So the 63 steps of fill and drain are
// paid once per run, not once per pair.  No LDS, no barrier, no atomics; every pair is the same sequence of fp32 operations
// wherever it runs, so a pair's bits do not depend on the batch around it.
#include "dtw.h"

// rule 2: difference, product and sum are separate fp32 operations (hipcc contracts a * b + c by default)
#pragma clang fp contract(off)

constexpr int DTW_FIRST = 1, DTW_LAST = 2;   // flags in the low bits of a row's tag; the query index sits above them

// lane l takes x of lane l - 1; lane 0, which has no such neighbour, takes lane0
__device__ __forceinline__ int dtw_shift(int lane0, int x) { return __builtin_amdgcn_update_dpp(lane0, x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ float dtw_shift(float lane0, float x) { return __int_as_float(dtw_shift(__float_as_int(lane0), __float_as_int(x))); }

template <int C, int F, bool WITH_K>
__global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(DtwArgs p) {
  const int lane = threadIdx.x & 63;
  const int task = __builtin_amdgcn_readfirstlane(blockIdx.x * DTW_WAVES + (threadIdx.x >> 6));
  if (task >= p.N * p.splits) return;
  const int q = task / p.splits, split = task % p.splits;
  const int p0 = (int)((long long)split * p.M / p.splits), p1 = (int)((long long)(split + 1) * p.M / p.splits);
  const float inf = __builtin_huge_valf();
  const int m = __builtin_amdgcn_readfirstlane(p.lens_b ? p.lens_b[q] : p.Lb);

  if (m < 1 || m > p.Lb) {   // rule 7: every pair of this reference
    for (int i = p0 + lane; i < p1; i += DTW_LANES) {
      if (p.dist) p.dist[(size_t)i * p.N + q] = inf;
      if (p.steps) p.steps[(size_t)i * p.N + q] = 0;
    }
    return;
  }

  float B[C][F];   // the lane's columns; columns at or past m are never read and hold 0 (they feed nothing that is written)
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int col = lane * C + c;
#pragma unroll
    for (int f = 0; f < F; ++f) B[c][f] = col < m ? p.b[((size_t)q * p.Lb + col) * F + f] : 0.f;
  }
  const int owner = (m - 1) / C, owner_col = (m - 1) % C;   // where D(., m - 1) lives

  float D[C], row[F], in_d_prev = inf;
  int K[C], in_k_prev = 0, tag = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) { D[c] = 0.f; K[c] = 0; }
#pragma unroll
  for (int f = 0; f < F; ++f) row[f] = 0.f;

  // queries p0 .. p1 - 1, then `owner` empty rows that push the last query's last row through to the owning lane
  for (int qi = p0; qi <= p1; ++qi) {
    const bool real = qi < p1;
    const int n = __builtin_amdgcn_readfirstlane(real ? (p.lens_a ? p.lens_a[qi] : p.La) : owner);
    if (real && (n < 1 || n > p.La)) {   // rule 7: this query takes no step
      if (lane == 0) {
        if (p.dist) p.dist[(size_t)qi * p.N + q] = inf;
        if (p.steps) p.steps[(size_t)qi * p.N + q] = 0;
      }
      continue;
    }
    for (int blk = 0; blk < n; blk += DTW_LANES) {
      float A[F];   // rows blk .. blk + 63 of the query, one per lane; rows at or past n are never read
#pragma unroll
      for (int f = 0; f < F; ++f) A[f] = (real && blk + lane < n) ? p.a[((size_t)qi * p.La + blk + lane) * F + f] : 0.f;
      const int count = n - blk < DTW_LANES ? n - blk : DTW_LANES;
      for (int s = 0; s < count; ++s) {
        const int i = blk + s;
        const int tag0 = real ? (qi << 2) | (i == 0 ? DTW_FIRST : 0) | (i == n - 1 ? DTW_LAST : 0) : 0;
        // the hand-off: the left neighbour's last column as it was one step ago, the query row and its tag
        const float in_d = dtw_shift(inf, D[C - 1]);
        const int in_k = WITH_K ? dtw_shift(0, K[C - 1]) : 0;
#pragma unroll
        for (int f = 0; f < F; ++f) row[f] = dtw_shift(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(A[f]), s)), row[f]);
        tag = dtw_shift(tag0, tag);

        float diag = in_d_prev, left = in_d;
        int k_diag = in_k_prev, k_left = in_k;
        if (tag & DTW_FIRST) {   // rules 3 and 4: no row above; D(0,0) = c(0,0) is "0 from the diagonal" with K 0
          diag = lane == 0 ? 0.f : inf;
          k_diag = 0;
#pragma unroll
          for (int c = 0; c < C; ++c) { D[c] = inf; K[c] = 0; }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float up = D[c];
          const int k_up = K[c];
          float cost = 0.f;
#pragma unroll
          for (int f = 0; f < F; ++f) {
            const float d = row[f] - B[c][f];
            const float d2 = d * d;
            cost = f == 0 ? d2 : cost + d2;
          }
          // the minimum and one addition are the whole loop-carried chain (left -> best -> d_new -> the next column's left);
          // rule 5 picks K beside it: the first of diagonal, i - 1, j - 1 that attains the minimum
          const float best = fminf(fminf(diag, up), left);
          const int k_best = WITH_K ? (diag == best ? k_diag : up == best ? k_up : k_left) : 0;
          const float d_new = cost + best;
          diag = up;
          k_diag = k_up;
          left = d_new;
          k_left = k_best + 1;
          D[c] = d_new;
          K[c] = k_left;
        }
        in_d_prev = in_d;
        in_k_prev = in_k;

        if ((tag & DTW_LAST) && lane == owner) {   // rule 6
          float d = D[0];
          int k = K[0];
#pragma unroll
          for (int c = 1; c < C; ++c)
            if (c == owner_col) { d = D[c]; k = K[c]; }
          const size_t o = (size_t)(tag >> 2) * p.N + q;
          if (p.normalize) d = d / (float)k;   // hipcc's default: a correctly rounded fp32 division
          if (p.dist) p.dist[o] = d;
          if (p.steps) p.steps[o] = k;
        }
      }
    }
  }
}

// rule 8: lane l scans q = l, l + 64, .. ascending and keeps the first smallest entry; the 64 candidates are joined by a
// butterfly that prefers the smaller index on a tie.  min is exact and the order of ties is by index: no order dependence.
__global__ __launch_bounds__(DTW_THREADS) void dtw_nearest_kernel(const float* __restrict__ dist, int M, int N, int skip_diag, float* __restrict__ nearest_out,
                                                                   int32_t* __restrict__ nearest_idx) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * DTW_WAVES + (threadIdx.x >> 6);
  if (r >= M) return;
  float best = __builtin_huge_valf();
  int bi = -1;
  for (int q = lane; q < N; q += DTW_LANES) {
    if (skip_diag && q == r) continue;
    const float v = dist[(size_t)r * N + q];
    if (v < best) { best = v; bi = q; }
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) {
    nearest_out[r] = best;
    if (nearest_idx) nearest_idx[r] = bi;
  }
}

template <int C, int F>
static void dtw_launch_cf(const DtwArgs& p, bool with_k, dim3 grid, hipStream_t st) {
  if (with_k) hipLaunchKernelGGL((dtw_kernel<C, F, true>), grid, dim3(DTW_THREADS), 0, st, p);
  else hipLaunchKernelGGL((dtw_kernel<C, F, false>), grid, dim3(DTW_THREADS), 0, st, p);
}

template <int C>
static void dtw_launch_c(const DtwArgs& p, int F, bool with_k, dim3 grid, hipStream_t st) {
  switch (F) {
    case 1: dtw_launch_cf<C, 1>(p, with_k, grid, st); break;
    case 2: dtw_launch_cf<C, 2>(p, with_k, grid, st); break;
    case 3: dtw_launch_cf<C, 3>(p, with_k, grid, st); break;
    default: dtw_launch_cf<C, 4>(p, with_k, grid, st); break;
  }
}

hipError_t launch_dtw(const DtwArgs& p, int F, int skip_diag, float* nearest_out, int32_t* nearest_idx, hipStream_t st) {
  const bool with_k = p.steps || p.normalize;   // the K carry is compiled out when nobody reads it
  const dim3 grid((p.N * p.splits + DTW_WAVES - 1) / DTW_WAVES);
  switch (dtw_cols(p.Lb)) {
    case 1: dtw_launch_c<1>(p, F, with_k, grid, st); break;
    case 2: dtw_launch_c<2>(p, F, with_k, grid, st); break;
    case 4: dtw_launch_c<4>(p, F, with_k, grid, st); break;
    case 8: dtw_launch_c<8>(p, F, with_k, grid, st); break;
    default: dtw_launch_c<16>(p, F, with_k, grid, st); break;
  }
  if (nearest_out)
    hipLaunchKernelGGL(dtw_nearest_kernel, dim3((p.M + DTW_WAVES - 1) / DTW_WAVES), dim3(DTW_THREADS), 0, st, p.dist, p.M, p.N, skip_diag, nearest_out,
                       nearest_idx);
  return hipGetLastError();
}
