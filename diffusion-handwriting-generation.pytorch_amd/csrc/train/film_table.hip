// film_table.hip — every AffineTransformLayer's gamma / beta Linear as one table: forward, weight gradient, sigma gradient.
#include <algorithm>

#include "../dhw_common.h"
#include "../dhw_kernels.h"
#include "train_common.h"

using namespace dhw_train;

namespace {

// All AffineTransformLayers' gamma / beta Linears (conditioning.py:16-18; 76 Linears of 32 inputs for num_layers = 2) as
// ONE launch each way.  Column j of the table film[B][TOT] belongs to output channel woff[j] / 32 of some Linear: its weight
// row starts at flat[woff[j]] (32 floats), its bias is flat[boff[j]] — the parameters stay where the state_dict puts them.
// (round 4: a thread owns one column for a chunk of samples — its 32 weights and its bias stay in registers, sigma is broadcast from
// LDS — instead of one block per sample re-reading every weight row: 12 -> ~5 us.  Same sum order per element as before.)
constexpr int FTB = 16;   // samples per block
__global__ __launch_bounds__(64) void film_table_fwd_kernel(const float* sigma, const float* flat, const int64_t* woff, const int64_t* boff, int B, int TOT,
                                                             float* film) {
  const int j = blockIdx.x * 64 + threadIdx.x, b0 = blockIdx.y * FTB, nb_ = min(FTB, B - b0);
  __shared__ float sg[FTB][32];
  for (int t = threadIdx.x; t < nb_ * 32; t += 64) sg[t >> 5][t & 31] = sigma[(b0 + (t >> 5)) * 32 + (t & 31)];
  __syncthreads();
  if (j >= TOT) return;
  const float* w = flat + woff[j];
  f32x4 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const f32x4*>(w + 4 * k);
  const float bias = flat[boff[j]];
  for (int b = 0; b < nb_; ++b) {
    float a = bias;
#pragma unroll
    for (int k = 0; k < 8; ++k) a += v[k][0] * sg[b][4 * k] + v[k][1] * sg[b][4 * k + 1] + v[k][2] * sg[b][4 * k + 2] + v[k][3] * sg[b][4 * k + 3];
    film[(long)(b0 + b) * TOT + j] = a;
  }
}
// dW[j][k] += sum_b dfilm[b][j] sigma[b][k];  db[j] += sum_b dfilm[b][j].  Block = 64 columns: the dfilm tile [32 samples][64] and
// sigma [32][32] go through LDS in coalesced passes, a thread = (column, 8 of the 32 k).  (One thread per (column, k) reading dfilm
// straight from memory fetched 8 useful bytes per wave-instruction: 30 us for 38 MFLOP.)
__global__ __launch_bounds__(256) void film_table_wgrad_kernel(const float* dfilm, const float* sigma, const int64_t* woff, const int64_t* boff, int B,
                                                                int TOT, float* gflat) {
  __shared__ float df[32][64], sg[32][32];
  const int t = threadIdx.x, jl = t & 63, kq = t >> 6, j0 = blockIdx.x * 64, j = j0 + jl;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sb = 0.f;
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int nb_ = min(32, B - b0);
    __syncthreads();
    // (unconditional clamped requests, all in flight before the first LDS store: see film_table_dgrad_kernel)
    float dv[8], sv[4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = t + u * 256, b = e >> 6, c = e & 63;
      dv[u] = dfilm[(long)(b0 + min(b, nb_ - 1)) * TOT + min(j0 + c, TOT - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = t + u * 256;
      sv[u] = sigma[(b0 + min(e >> 5, nb_ - 1)) * 32 + (e & 31)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = t + u * 256, b = e >> 6, c = e & 63;
      df[b][c] = b < nb_ && j0 + c < TOT ? dv[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = t + u * 256;
      sg[e >> 5][e & 31] = (e >> 5) < nb_ ? sv[u] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int b = 0; b < 32; ++b) {
      const float d = df[b][jl];
      sb += d;
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += d * sg[b][8 * kq + k];
    }
  }
  if (j >= TOT) return;
  float* gw = gflat + woff[j] + 8 * kq;
#pragma unroll
  for (int k = 0; k < 8; ++k) gw[k] += s[k];
  if (kq == 0) gflat[boff[j]] += sb;
}
// dsigma[b][k] += sum_j dfilm[b][j] W[j][k]: block = FTD columns for 32 samples; the weight rows of the chunk ([FTD][32]) and the
// dfilm tile ([32][FTD]) through LDS once, a thread = (sample, 4 of the 32 k), four atomics per thread.  (One block per (sample,
// chunk) re-read the chunk's weight rows for every sample: 76 MB of L2 reads for a 2.4 MB matrix, 19 us.)
constexpr int FTD = 64;   // (290 column chunks for the 18 560 columns of num_layers = 2, walked by 64 workgroups)
__global__ __launch_bounds__(256) void film_table_dgrad_kernel(const float* dfilm, const float* flat, const int64_t* woff, int B, int TOT, float* dsigma) {
  __shared__ __attribute__((aligned(16))) float W[FTD][36];
  __shared__ float df[32][FTD + 1];
  const int t = threadIdx.x, b0 = blockIdx.y * 32, nb_ = min(32, B - b0);
  const int b = t >> 3, kq = t & 7;
  f32x4 s = (f32x4){0, 0, 0, 0};
  // (round 5: a workgroup walks over several column chunks and adds its 1 024 partial sums to dsigma ONCE — 290 workgroups x 1 024 atomics on the same
  // 1 024 addresses were 25 of the kernel's 31 us; every request unconditional at a clamped address, all of a pass in flight before its first LDS store)
  for (int j0 = blockIdx.x * FTD; j0 < TOT; j0 += gridDim.x * FTD) {
    const int nj = min(FTD, TOT - j0);
    int64_t wo[FTD * 8 / 256];
#pragma unroll
    for (int u = 0; u < FTD * 8 / 256; ++u) wo[u] = woff[j0 + min((t + u * 256) >> 3, nj - 1)];
    float dv[32 * FTD / 256];
#pragma unroll
    for (int u = 0; u < 32 * FTD / 256; ++u) {
      const int e = t + u * 256, bb = e / FTD, c = e - bb * FTD;
      dv[u] = dfilm[(long)(b0 + min(bb, nb_ - 1)) * TOT + j0 + min(c, nj - 1)];
    }
    f32x4 wv[FTD * 8 / 256];
#pragma unroll
    for (int u = 0; u < FTD * 8 / 256; ++u) wv[u] = *reinterpret_cast<const f32x4*>(flat + wo[u] + 4 * ((t + u * 256) & 7));
    __syncthreads();   // (the previous chunk's tiles have been read)
#pragma unroll
    for (int u = 0; u < 32 * FTD / 256; ++u) {
      const int e = t + u * 256, bb = e / FTD, c = e - bb * FTD;
      df[bb][c] = bb < nb_ && c < nj ? dv[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < FTD * 8 / 256; ++u) {
      const int e = t + u * 256, c = e >> 3, k4 = e & 7;
      *reinterpret_cast<f32x4*>(&W[c][4 * k4]) = c < nj ? wv[u] : (f32x4){0, 0, 0, 0};
    }
    __syncthreads();
#pragma unroll 8
    for (int c = 0; c < FTD; ++c) s += df[b][c] * *reinterpret_cast<const f32x4*>(&W[c][4 * kq]);
  }
  if (b < nb_) {
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(dsigma + (b0 + b) * 32 + 4 * kq + k, s[k]);
  }
}

}  // namespace

hipError_t launch_film_table(int dir, const float* sigma, const float* flat, const int64_t* woff, const int64_t* boff, int B, int TOT, float* film,
                             float* gflat, float* dsigma, hipStream_t st) {
  if (dir == 0) {
    hipLaunchKernelGGL(film_table_fwd_kernel, dim3(nb(TOT, 64), nb(B, FTB)), dim3(64), 0, st, sigma, flat, woff, boff, B, TOT, film);
  } else {
    hipLaunchKernelGGL(film_table_wgrad_kernel, dim3(nb(TOT, 64)), dim3(256), 0, st, film, sigma, woff, boff, B, TOT, gflat);
    hipLaunchKernelGGL(film_table_dgrad_kernel, dim3(std::min<unsigned>(nb(TOT, FTD), 64u), nb(B, 32)), dim3(256), 0, st, film, flat, woff, B, TOT, dsigma);
  }
  return hipGetLastError();
}
