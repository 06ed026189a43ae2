// elementwise.hip — the training step's passes over [rows, C] fp32 activations (dhw_train.h "dhw_op_*"): activations, adds, FiLM,
// LayerNorm, softmax, AvgPool / upsampling, embedding, dropout masks, each with its adjoint; the fused FiLM / LayerNorm chains; the
// 16-byte forms; and the launchers that choose between the scalar and the 16-byte form.
#include <cstdlib>
#include <initializer_list>

#include "../dhw_common.h"
#include "../dhw_kernels.h"
#include "train_common.h"

using namespace dhw_train;

namespace {

__global__ __launch_bounds__(256) void unary_kernel(int kind, const float* x, long n, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  y[i] = kind == 0 ? silu_f(v) : sigmoid_f(v);
}
// kind 0: dx (+)= dy * SiLU'(x);  kind 1: dx (+)= dy * y (1 - y) with y = sigmoid output passed as x
__global__ __launch_bounds__(256) void unary_bwd_kernel(int kind, const float* dy, const float* x, long n, float* dx, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = kind == 0 ? dy[i] * dsilu_f(x[i]) : dy[i] * x[i] * (1.0f - x[i]);
  dx[i] = accumulate ? dx[i] + v : v;
}
// out = a + b (b may be null: copy);  accumulate: out += a (+ b)
__global__ __launch_bounds__(256) void add_kernel2(const float* a, const float* b, long n, float* out, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = a[i] + (b ? b[i] : 0.f);
  out[i] = accumulate ? out[i] + v : v;
}
// out[b][l][c] = x[b][l][c] + table[l][c]   (positional encodings: a constant, no gradient)
__global__ __launch_bounds__(256) void add_rows_kernel(const float* x, const float* table, long n, long per_sample, float* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = x[i] + table[i % per_sample];
}
// y = x * gamma[b] + beta[b] (per-sample [B][C] rows at given strides)
__global__ __launch_bounds__(256) void film_fwd_kernel(const float* x, const float* gam, const float* bet, long pstride, int L, int C, long n, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long r = i / C;
  const int c = (int)(i - r * C), b = (int)(r / L);
  y[i] = x[i] * gam[b * pstride + c] + bet[b * pstride + c];
}
// LayerNorm(eps 1e-6, no affine) over the C channels of each row; one wave per row; keeps mean / rstd for the backward
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* x, long rows, int C, float* y, float* mean_out, float* rstd_out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; v += d * d; }
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  const float rstd = rsqrtf(v / C + 1e-6f);
  for (int c = lane; c < C; c += 64) y[row * C + c] = (xr[c] - mean) * rstd;
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}
// dx (+)= rstd * (dy - mean(dy) - y * mean(dy * y)),  y = the normalised output
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* dy, const float* y, const float* rstd, long rows, int C, float* dx, int accumulate) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* d = dy + row * C;
  const float* yr = y + row * C;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < C; c += 64) { s1 += d[c]; s2 += d[c] * yr[c]; }
  for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
  s1 /= C; s2 /= C;
  const float r = rstd[row];
  for (int c = lane; c < C; c += 64) {
    const float v = r * (d[c] - s1 - yr[c] * s2);
    dx[row * C + c] = accumulate ? dx[row * C + c] + v : v;
  }
}
// P = softmax(S * scale + mask[b][key] * (-1e9)) over the `cols` keys of each row; rows are [B][H][Lq], mask [B][cols] or null
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* s, long rows, int cols, long rows_per_sample, const float* mask, float scale, float* p) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* sr = s + row * cols;
  const float* mr = mask ? mask + (row / rows_per_sample) * cols : nullptr;
  float mx = -INFINITY;
  for (int c = lane; c < cols; c += 64) mx = fmaxf(mx, sr[c] * scale + (mr ? mr[c] * -1e9f : 0.f));
  for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
  for (int c = lane; c < cols; c += 64) sum += expf(sr[c] * scale + (mr ? mr[c] * -1e9f : 0.f) - mx);
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  for (int c = lane; c < cols; c += 64) p[row * cols + c] = expf(sr[c] * scale + (mr ? mr[c] * -1e9f : 0.f) - mx) / sum;
}
// dS = scale * P * (dP - sum_key(dP * P))
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* dp, const float* p, long rows, int cols, float scale, float* ds) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += dp[row * cols + c] * p[row * cols + c];
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  for (int c = lane; c < cols; c += 64) ds[row * cols + c] = scale * p[row * cols + c] * (dp[row * cols + c] - s);
}
// AvgPool1d(2) over rows / its backward;  nearest x2 upsampling / its backward  (rows C-last, L even)
__global__ __launch_bounds__(256) void pool_kernel(int mode, const float* x, long n_out, int C, float* y, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  const long r = i / C;
  const int c = (int)(i - r * C);
  float v;
  if (mode == 0) v = 0.5f * (x[(2 * r) * C + c] + x[(2 * r + 1) * C + c]);      // pool fwd: out row r <- rows 2r, 2r+1
  else if (mode == 1) v = 0.5f * x[(r / 2) * C + c];                              // pool bwd: dx row r <- 0.5 dy[r/2]
  else if (mode == 2) v = x[(r / 2) * C + c];                                     // upsample fwd: out row r <- row r/2
  else v = x[(2 * r) * C + c] + x[(2 * r + 1) * C + c];                           // upsample bwd: dx row r <- dy[2r] + dy[2r+1]
  y[i] = accumulate ? y[i] + v : v;
}
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* ids, const float* table, long n, int C, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = table[ids[i / C] * C + i % C];
}
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int64_t* ids, const float* dy, long n, int C, float* dtable) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) atomicAdd(dtable + ids[i / C] * C + i % C, dy[i]);
}
// y = x * mask * scale (dropout with a supplied keep-mask; also its own backward)
__global__ __launch_bounds__(256) void mask_mul_kernel(const float* x, const float* mask, float scale, long n, float* y, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i] * mask[i] * scale;
  y[i] = accumulate ? y[i] + v : v;
}
// FiLM backward without activation for per-sample [B][C] parameter rows: du (+)= d * gamma, dgamma[b][c] += sum_l d u, dbeta += sum_l d
__global__ __launch_bounds__(256) void film_bwd2_kernel(const float* d, const float* u, const float* gam, long pstride, int L, int C, float* du, int accumulate,
                                                         float* dgam, float* dbet) {
  // block = 64 channels x 4 row groups over a 64-row chunk of one sample; per-(block, channel) partial sums go out as atomics
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6, b = blockIdx.y;
  const int l0 = blockIdx.z * 64, l1 = min(L, l0 + 64);
  float sg = 0.f, sb = 0.f;
  if (c < C) {
    const float ga = gam[b * pstride + c];
    for (int l = l0 + rg; l < l1; l += 4) {
      const long e = ((long)b * L + l) * C + c;
      const float dd = d[e];
      sg += dd * u[e];
      sb += dd;
      du[e] = accumulate ? du[e] + dd * ga : dd * ga;
    }
  }
  __shared__ float rs[256], rb[256];
  rs[threadIdx.x] = sg;
  rb[threadIdx.x] = sb;
  __syncthreads();
  if (rg == 0 && c < C) {
    const int x = threadIdx.x;
    atomicAdd(dgam + b * pstride + c, rs[x] + rs[x + 64] + rs[x + 128] + rs[x + 192]);
    atomicAdd(dbet + b * pstride + c, rb[x] + rb[x + 64] + rb[x + 128] + rb[x + 192]);
  }
}

// ---- fused element-wise chains (round 3): the element-wise launches of the op-by-op tape are HBM-bound passes over
// [rows, C] fp32 activations (5-10 us each, ~25 % of an update); FiLM -> SiLU and LayerNorm -> FiLM are evaluated in ONE pass
// each way, the intermediate (FiLM output / normalised rows) is recomputed in the backward instead of stored and re-read.
// y = act ? SiLU(x gamma[b] + beta[b]) : x gamma[b] + beta[b];   4 channels per thread (C % 4 == 0)
__global__ __launch_bounds__(256) void film_act_fwd_kernel(const float* x, const float* gam, const float* bet, long pstride, int L, int C, long n4,
                                                            int act, const float* addend, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long e = i * 4, r = e / C;
  const int c = (int)(e - r * C), b = (int)(r / L);
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
  const f32x4 ga = *reinterpret_cast<const f32x4*>(gam + b * pstride + c), be = *reinterpret_cast<const f32x4*>(bet + b * pstride + c);
  f32x4 a = v * ga + be;
  if (act) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = silu_f(a[k]);
  }
  if (addend) a += *reinterpret_cast<const f32x4*>(addend + e);   // (a residual add riding on the pass)
  *reinterpret_cast<f32x4*>(y + e) = a;
}
// backward of the above: d' = act ? dy * SiLU'(x gamma + beta) : dy;  dx (+)= d' gamma;  dgamma[b][c] += sum_l d' x;  dbeta[b][c] += sum_l d'
// (block = 64 channels x 4 row groups over a 64-row chunk of one sample, as film_bwd2_kernel)
__global__ __launch_bounds__(256) void film_act_bwd_kernel(const float* d, const float* u, const float* gam, const float* bet, long pstride, int L, int C,
                                                            int act, float* du, int accumulate, float* dgam, float* dbet) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6, b = blockIdx.y;
  const int l0 = blockIdx.z * 64, l1 = min(L, l0 + 64);
  float sg = 0.f, sb = 0.f;
  if (c < C) {
    const float ga = gam[b * pstride + c], be = bet[b * pstride + c];
    for (int l = l0 + rg; l < l1; l += 4) {
      const long e = ((long)b * L + l) * C + c;
      const float x = u[e];
      float dd = d[e];
      if (act) dd *= dsilu_f(x * ga + be);
      sg += dd * x;
      sb += dd;
      du[e] = accumulate ? du[e] + dd * ga : dd * ga;
    }
  }
  __shared__ float rs[256], rb[256];
  rs[threadIdx.x] = sg;
  rb[threadIdx.x] = sb;
  __syncthreads();
  if (rg == 0 && c < C) {
    const int x = threadIdx.x;
    atomicAdd(dgam + b * pstride + c, rs[x] + rs[x + 64] + rs[x + 128] + rs[x + 192]);
    atomicAdd(dbet + b * pstride + c, rb[x] + rb[x + 64] + rb[x + 128] + rb[x + 192]);
  }
}
// y = LayerNorm(x) gamma[b] + beta[b]  (eps 1e-6, no LN affine; one wave per row; mean / rstd kept for the backward)
__global__ __launch_bounds__(256) void ln_film_fwd_kernel(const float* x, long rows, int C, const float* gam, const float* bet, long pstride, int L,
                                                           const float* addend, float* y, float* act_out, const float* pe, float* pe_out, float* mean_out, float* rstd_out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * C;
  const long pb = (row / L) * pstride;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; v += d * d; }
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  const float rstd = rsqrtf(v / C + 1e-6f);
  for (int c = lane; c < C; c += 64) {
    const float v = (xr[c] - mean) * rstd * gam[pb + c] + bet[pb + c] + (addend ? addend[row * C + c] : 0.f);
    y[row * C + c] = v;
    if (act_out) act_out[row * C + c] = silu_f(v);   // (the SiLU an ff_network opens with, utils/nn.py:145)
    if (pe_out) pe_out[row * C + c] = v + pe[(row % L) * C + c];   // (x + PE: what the q / k projections of the next attention take, model.py:41-48)
  }
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}
// backward: xn = (x - mean) rstd;  dn = dy gamma;  dx (+)= rstd (dn - mean(dn) - xn mean(dn xn));  dgamma[b][c] += sum_l dy xn;  dbeta += sum_l dy.
// grid (ceil(L / 8), B): a block's 4 waves take 2 rows each of one sample (8-row chunks keep >= 1 000 blocks in flight at the
// stroke levels; 64-row chunks ran at 43 us per launch), per-lane channel partial sums in registers (C <= 64 * 8), then one LDS
// reduction and one atomic per channel and block.
__global__ __launch_bounds__(256) void ln_film_bwd_kernel(const float* dy, const float* x, const float* mean, const float* rstd, const float* gam, long pstride,
                                                           int L, int C, float* dx, int accumulate, float* dgam, float* dbet) {
  constexpr int KMAX = 8;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  const int l0 = blockIdx.x * 8, l1 = min(L, l0 + 8);
  float sg[KMAX], sb[KMAX], ga[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { sg[k] = 0.f; sb[k] = 0.f; ga[k] = lane + 64 * k < C ? gam[b * pstride + lane + 64 * k] : 0.f; }
  for (int l = l0 + w; l < l1; l += 4) {
    const long row = (long)b * L + l;
    const float mu = mean[row], rs = rstd[row];
    float xn[KMAX], dn[KMAX], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = lane + 64 * k;
      const bool in = c < C;
      const float d = in ? dy[row * C + c] : 0.f;
      xn[k] = in ? (x[row * C + c] - mu) * rs : 0.f;
      dn[k] = d * ga[k];
      sg[k] += d * xn[k];
      sb[k] += d;
      s1 += dn[k];
      s2 += dn[k] * xn[k];
    }
    for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    s1 /= C; s2 /= C;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = lane + 64 * k;
      if (c < C) {
        const float v = rs * (dn[k] - s1 - xn[k] * s2);
        dx[row * C + c] = accumulate ? dx[row * C + c] + v : v;
      }
    }
  }
  __shared__ float red[2][4][64 * KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { red[0][w][lane + 64 * k] = sg[k]; red[1][w][lane + 64 * k] = sb[k]; }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    atomicAdd(dgam + b * pstride + c, red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c]);
    atomicAdd(dbet + b * pstride + c, red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c]);
  }
}

// ---- 16-byte forms of the three passes above (round 4): C % 4 == 0, C <= 512, every pointer and row 16-byte aligned (the launchers
// check and fall back).  A lane holds channels 4 * lane + 256 * k .. + 3 (k < 2), a row is read once into registers; the scalar forms
// moved 4 bytes per lane and instruction and re-read the row for each of LayerNorm's passes (8-10 us per launch against 5-6 us of
// memory time, rocprofv3 trace of tools/bench_train.py).  Same element-wise arithmetic; the reductions associate differently.

__global__ __launch_bounds__(256) void ln_film_fwd4_kernel(const float* x, long rows, int C, const float* gam, const float* bet, long pstride, int L,
                                                            const float* addend, float* y, float* act_out, const float* pe, float* pe_out, float* mean_out, float* rstd_out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long pb = (row / L) * pstride;
  f32x4 v[2];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = 4 * lane + 256 * k;
    v[k] = c < C ? ld4(x + row * C + c) : (f32x4){0, 0, 0, 0};
    s += sum4(v[k]);
  }
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / C;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (4 * lane + 256 * k < C) { const f32x4 d = v[k] - mean; q += sum4(d * d); }
  for (int o = 32; o; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = rsqrtf(q / C + 1e-6f);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < C) {
      f32x4 o = (v[k] - mean) * rstd * ld4(gam + pb + c) + ld4(bet + pb + c);
      if (addend) o += ld4(addend + row * C + c);
      *reinterpret_cast<f32x4*>(y + row * C + c) = o;
      if (act_out) *reinterpret_cast<f32x4*>(act_out + row * C + c) = (f32x4){silu_f(o[0]), silu_f(o[1]), silu_f(o[2]), silu_f(o[3])};
      if (pe_out) *reinterpret_cast<f32x4*>(pe_out + row * C + c) = o + ld4(pe + (row % L) * C + c);
    }
  }
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}

__global__ __launch_bounds__(256) void ln_film_bwd4_kernel(const float* dy, const float* x, const float* mean, const float* rstd, const float* gam, long pstride,
                                                            int L, int C, float* dx, int accumulate, float* dgam, float* dbet) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  const int l0 = blockIdx.x * 8, l1 = min(L, l0 + 8);
  const f32x4 z4 = (f32x4){0, 0, 0, 0};
  f32x4 sg[2] = {z4, z4}, sb[2] = {z4, z4}, ga[2];
  bool in[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    in[k] = 4 * lane + 256 * k < C;
    ga[k] = in[k] ? ld4(gam + b * pstride + 4 * lane + 256 * k) : z4;
  }
  for (int l = l0 + w; l < l1; l += 4) {
    const long row = (long)b * L + l;
    const float mu = mean[row], rs = rstd[row];
    f32x4 xn[2], dn[2];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = 4 * lane + 256 * k;
      const f32x4 d = in[k] ? ld4(dy + row * C + c) : z4;
      xn[k] = in[k] ? (ld4(x + row * C + c) - mu) * rs : z4;
      dn[k] = d * ga[k];
      sg[k] += d * xn[k];
      sb[k] += d;
      s1 += sum4(dn[k]);
      s2 += sum4(dn[k] * xn[k]);
    }
    for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    s1 /= C; s2 /= C;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = 4 * lane + 256 * k;
      if (in[k]) {
        f32x4 v = rs * (dn[k] - s1 - xn[k] * s2);
        if (accumulate) v += ld4(dx + row * C + c);
        *reinterpret_cast<f32x4*>(dx + row * C + c) = v;
      }
    }
  }
  __shared__ __attribute__((aligned(16))) float red[2][4][512];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    *reinterpret_cast<f32x4*>(&red[0][w][4 * lane + 256 * k]) = sg[k];
    *reinterpret_cast<f32x4*>(&red[1][w][4 * lane + 256 * k]) = sb[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    atomicAdd(dgam + b * pstride + c, red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c]);
    atomicAdd(dbet + b * pstride + c, red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c]);
  }
}

// (block = 16 lanes x 4 channels = 64 channels, 16 row groups over a 64-row chunk of one sample)
__global__ __launch_bounds__(256) void film_act_bwd4_kernel(const float* d, const float* u, const float* gam, const float* bet, long pstride, int L, int C,
                                                             int act, float* du, int accumulate, float* dgam, float* dbet) {
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4, c = blockIdx.x * 64 + 4 * cl, b = blockIdx.y;
  const int l0 = blockIdx.z * 64, l1 = min(L, l0 + 64);
  f32x4 sg = (f32x4){0, 0, 0, 0}, sb = sg;
  if (c < C) {
    const f32x4 ga = ld4(gam + b * pstride + c), be = ld4(bet + b * pstride + c);
    for (int l = l0 + rg; l < l1; l += 16) {
      const long e = ((long)b * L + l) * C + c;
      const f32x4 x = ld4(u + e);
      f32x4 dd = ld4(d + e);
      if (act) {
        const f32x4 a = x * ga + be;
        dd *= (f32x4){dsilu_f(a[0]), dsilu_f(a[1]), dsilu_f(a[2]), dsilu_f(a[3])};
      }
      sg += dd * x;
      sb += dd;
      f32x4 o = dd * ga;
      if (accumulate) o += ld4(du + e);
      *reinterpret_cast<f32x4*>(du + e) = o;
    }
  }
  __shared__ __attribute__((aligned(16))) float rs[16][64], rb[16][64];
  *reinterpret_cast<f32x4*>(&rs[rg][4 * cl]) = sg;
  *reinterpret_cast<f32x4*>(&rb[rg][4 * cl]) = sb;
  __syncthreads();
  const int x = threadIdx.x;
  if (x < 64 && blockIdx.x * 64 + x < C) {
    float a = 0.f, bsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a += rs[r][x]; bsum += rb[r][x]; }
    atomicAdd(dgam + b * pstride + blockIdx.x * 64 + x, a);
    atomicAdd(dbet + b * pstride + blockIdx.x * 64 + x, bsum);
  }
}

// ---- 16-byte forms of the one-float-per-thread passes (same precondition: n, C multiples of 4, aligned bases)
__global__ __launch_bounds__(256) void unary4_kernel(int kind, const float* x, long n4, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 v = ld4(x + 4 * i);
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = kind == 0 ? silu_f(v[k]) : sigmoid_f(v[k]);
  *reinterpret_cast<f32x4*>(y + 4 * i) = o;
}
__global__ __launch_bounds__(256) void add4_kernel(const float* a, const float* b, long n4, float* out, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = ld4(a + 4 * i);
  if (b) v += ld4(b + 4 * i);
  if (accumulate) v += ld4(out + 4 * i);
  *reinterpret_cast<f32x4*>(out + 4 * i) = v;
}
__global__ __launch_bounds__(256) void add_rows4_kernel(const float* x, const float* table, long n4, long per_sample4, float* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) *reinterpret_cast<f32x4*>(out + 4 * i) = ld4(x + 4 * i) + ld4(table + 4 * (i % per_sample4));
}
__global__ __launch_bounds__(256) void mask_mul4_kernel(const float* x, const float* mask, float scale, long n4, float* y, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = ld4(x + 4 * i) * ld4(mask + 4 * i) * scale;
  if (accumulate) v += ld4(y + 4 * i);
  *reinterpret_cast<f32x4*>(y + 4 * i) = v;
}
// (a block = 256 / (C / 4) whole output rows, a thread = 4 channels of one of them: one 32-bit division per thread)
__global__ __launch_bounds__(256) void pool4_kernel(int mode, const float* x, int C, long rows, float* y, int accumulate) {
  const int c4 = C / 4, rpb = 256 / c4, rr = threadIdx.x / c4;
  const long r = (long)blockIdx.x * rpb + rr;
  const int c = 4 * (threadIdx.x - rr * c4);
  if (rr >= rpb || r >= rows) return;
  f32x4 v;
  if (mode == 0) v = 0.5f * (ld4(x + (2 * r) * C + c) + ld4(x + (2 * r + 1) * C + c));
  else if (mode == 1) v = 0.5f * ld4(x + (r / 2) * C + c);
  else if (mode == 2) v = ld4(x + (r / 2) * C + c);
  else v = ld4(x + (2 * r) * C + c) + ld4(x + (2 * r + 1) * C + c);
  if (accumulate) v += ld4(y + r * C + c);
  *reinterpret_cast<f32x4*>(y + r * C + c) = v;
}
// softmax over rows of <= 256 columns held in registers (one exponential per element instead of three evaluations, one read of s)
__global__ __launch_bounds__(256) void softmax_fwd_r_kernel(const float* s, long rows, int cols, long rows_per_sample, const float* mask, float scale, float* p) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* sr = s + row * cols;
  const float* mr = mask ? mask + (row / rows_per_sample) * cols : nullptr;
  float v[4], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < cols ? sr[c] * scale + (mr ? mr[c] * -1e9f : 0.f) : -INFINITY;
    mx = fmaxf(mx, v[k]);
  }
  for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = lane + 64 * k < cols ? expf(v[k] - mx) : 0.f;
    sum += v[k];
  }
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < cols) p[row * cols + lane + 64 * k] = v[k] / sum;
}
__global__ __launch_bounds__(256) void softmax_bwd_r_kernel(const float* dp, const float* p, long rows, int cols, float scale, float* ds) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float a[4], b[4], s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    a[k] = c < cols ? dp[row * cols + c] : 0.f;
    b[k] = c < cols ? p[row * cols + c] : 0.f;
    s += a[k] * b[k];
  }
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < cols) ds[row * cols + lane + 64 * k] = scale * b[k] * (a[k] - s);
}

}  // namespace

// the 16-byte kernels' precondition: whole f32x4 per lane (C, the table's row stride) and 16-byte aligned bases (null = absent).
// DHW_TRAIN_VEC4=0: the scalar forms everywhere (A/B)
static bool vec4_ok(int C, long pstride, std::initializer_list<const void*> ptrs) {
  static const bool off = [] { const char* e = getenv("DHW_TRAIN_VEC4"); return e && atoi(e) == 0; }();
  if (off || C % 4 || pstride % 4) return false;
  for (const void* q : ptrs)
    if (reinterpret_cast<uintptr_t>(q) & 15) return false;
  return true;
}
hipError_t launch_unary(int kind, const float* x, long n, float* y, hipStream_t st) {
  if (n % 4 == 0 && vec4_ok(4, 0, {x, y})) hipLaunchKernelGGL(unary4_kernel, dim3(nb(n / 4)), dim3(256), 0, st, kind, x, n / 4, y);
  else hipLaunchKernelGGL(unary_kernel, dim3(nb(n)), dim3(256), 0, st, kind, x, n, y);
  return hipGetLastError();
}
hipError_t launch_unary_bwd(int kind, const float* dy, const float* x, long n, float* dx, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(unary_bwd_kernel, dim3(nb(n)), dim3(256), 0, st, kind, dy, x, n, dx, accumulate);
  return hipGetLastError();
}
hipError_t launch_add2(const float* a, const float* b, long n, float* out, int accumulate, hipStream_t st) {
  if (n % 4 == 0 && vec4_ok(4, 0, {a, b, out})) hipLaunchKernelGGL(add4_kernel, dim3(nb(n / 4)), dim3(256), 0, st, a, b, n / 4, out, accumulate);
  else hipLaunchKernelGGL(add_kernel2, dim3(nb(n)), dim3(256), 0, st, a, b, n, out, accumulate);
  return hipGetLastError();
}
hipError_t launch_add_rows(const float* x, const float* table, long n, long per_sample, float* out, hipStream_t st) {
  if (n % 4 == 0 && per_sample % 4 == 0 && vec4_ok(4, 0, {x, table, out}))
    hipLaunchKernelGGL(add_rows4_kernel, dim3(nb(n / 4)), dim3(256), 0, st, x, table, n / 4, per_sample / 4, out);
  else hipLaunchKernelGGL(add_rows_kernel, dim3(nb(n)), dim3(256), 0, st, x, table, n, per_sample, out);
  return hipGetLastError();
}
hipError_t launch_film_fwd(const float* x, const float* gam, const float* bet, long pstride, int B, int L, int C, float* y, hipStream_t st) {
  const long n = (long)B * L * C;
  hipLaunchKernelGGL(film_fwd_kernel, dim3(nb(n)), dim3(256), 0, st, x, gam, bet, pstride, L, C, n, y);
  return hipGetLastError();
}
hipError_t launch_film_bwd2(const float* d, const float* u, const float* gam, long pstride, int B, int L, int C, float* du, int accumulate, float* dgam,
                            float* dbet, hipStream_t st) {
  hipLaunchKernelGGL(film_bwd2_kernel, dim3(nb(C, 64), B, nb(L, 64)), dim3(256), 0, st, d, u, gam, pstride, L, C, du, accumulate, dgam, dbet);
  return hipGetLastError();
}
hipError_t launch_film_act_fwd(const float* x, const float* gam, const float* bet, long pstride, int B, int L, int C, int act, const float* addend, float* y,
                               hipStream_t st) {
  const long n4 = (long)B * L * C / 4;
  hipLaunchKernelGGL(film_act_fwd_kernel, dim3(nb(n4)), dim3(256), 0, st, x, gam, bet, pstride, L, C, n4, act, addend, y);
  return hipGetLastError();
}
hipError_t launch_film_act_bwd(const float* d, const float* u, const float* gam, const float* bet, long pstride, int B, int L, int C, int act, float* du,
                               int accumulate, float* dgam, float* dbet, hipStream_t st) {
  if (vec4_ok(C, pstride, {d, u, gam, bet, du}))
    hipLaunchKernelGGL(film_act_bwd4_kernel, dim3(nb(C, 64), B, nb(L, 64)), dim3(256), 0, st, d, u, gam, bet, pstride, L, C, act, du, accumulate, dgam, dbet);
  else
    hipLaunchKernelGGL(film_act_bwd_kernel, dim3(nb(C, 64), B, nb(L, 64)), dim3(256), 0, st, d, u, gam, bet, pstride, L, C, act, du, accumulate, dgam, dbet);
  return hipGetLastError();
}
hipError_t launch_ln_film_fwd(const float* x, long rows, int C, const float* gam, const float* bet, long pstride, int L, const float* addend, float* y,
                              float* act_out, const float* pe, float* pe_out, float* mean, float* rstd, hipStream_t st) {
  if (C <= 512 && vec4_ok(C, pstride, {x, gam, bet, addend, y, act_out, pe, pe_out}))
    hipLaunchKernelGGL(ln_film_fwd4_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, x, rows, C, gam, bet, pstride, L, addend, y, act_out, pe, pe_out, mean, rstd);
  else
    hipLaunchKernelGGL(ln_film_fwd_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, x, rows, C, gam, bet, pstride, L, addend, y, act_out, pe, pe_out, mean, rstd);
  return hipGetLastError();
}
hipError_t launch_ln_film_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gam, long pstride, int B, int L, int C,
                              float* dx, int accumulate, float* dgam, float* dbet, hipStream_t st) {
  if (C <= 512 && vec4_ok(C, pstride, {dy, x, gam, dx}))
    hipLaunchKernelGGL(ln_film_bwd4_kernel, dim3(nb(L, 8), B), dim3(256), 0, st, dy, x, mean, rstd, gam, pstride, L, C, dx, accumulate, dgam, dbet);
  else
    hipLaunchKernelGGL(ln_film_bwd_kernel, dim3(nb(L, 8), B), dim3(256), 0, st, dy, x, mean, rstd, gam, pstride, L, C, dx, accumulate, dgam, dbet);
  return hipGetLastError();
}
hipError_t launch_ln_fwd(const float* x, long rows, int C, float* y, float* mean, float* rstd, hipStream_t st) {
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, x, rows, C, y, mean, rstd);
  return hipGetLastError();
}
hipError_t launch_ln_bwd(const float* dy, const float* y, const float* rstd, long rows, int C, float* dx, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, dy, y, rstd, rows, C, dx, accumulate);
  return hipGetLastError();
}
hipError_t launch_softmax_fwd(const float* s, long rows, int cols, long rows_per_sample, const float* mask, float scale, float* p, hipStream_t st) {
  if (cols <= 256) hipLaunchKernelGGL(softmax_fwd_r_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, s, rows, cols, rows_per_sample, mask, scale, p);
  else hipLaunchKernelGGL(softmax_fwd_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, s, rows, cols, rows_per_sample, mask, scale, p);
  return hipGetLastError();
}
hipError_t launch_softmax_bwd(const float* dp, const float* p, long rows, int cols, float scale, float* ds, hipStream_t st) {
  if (cols <= 256) hipLaunchKernelGGL(softmax_bwd_r_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, dp, p, rows, cols, scale, ds);
  else hipLaunchKernelGGL(softmax_bwd_kernel, dim3(nb(rows, 4)), dim3(256), 0, st, dp, p, rows, cols, scale, ds);
  return hipGetLastError();
}
hipError_t launch_pool(int mode, const float* x, long n_out, int C, float* y, int accumulate, hipStream_t st) {
  if (n_out % C == 0 && C <= 1024 && vec4_ok(C, 0, {x, y}))
    hipLaunchKernelGGL(pool4_kernel, dim3(nb(n_out / C, 256 / (C / 4))), dim3(256), 0, st, mode, x, C, n_out / C, y, accumulate);
  else hipLaunchKernelGGL(pool_kernel, dim3(nb(n_out)), dim3(256), 0, st, mode, x, n_out, C, y, accumulate);
  return hipGetLastError();
}
hipError_t launch_embed(int bwd, const int64_t* ids, const float* src, long n, int C, float* dst, hipStream_t st) {
  if (bwd) hipLaunchKernelGGL(embed_bwd_kernel, dim3(nb(n)), dim3(256), 0, st, ids, src, n, C, dst);
  else hipLaunchKernelGGL(embed_fwd_kernel, dim3(nb(n)), dim3(256), 0, st, ids, src, n, C, dst);
  return hipGetLastError();
}
hipError_t launch_mask_mul(const float* x, const float* mask, float scale, long n, float* y, int accumulate, hipStream_t st) {
  if (n % 4 == 0 && vec4_ok(4, 0, {x, mask, y})) hipLaunchKernelGGL(mask_mul4_kernel, dim3(nb(n / 4)), dim3(256), 0, st, x, mask, scale, n / 4, y, accumulate);
  else hipLaunchKernelGGL(mask_mul_kernel, dim3(nb(n)), dim3(256), 0, st, x, mask, scale, n, y, accumulate);
  return hipGetLastError();
}
