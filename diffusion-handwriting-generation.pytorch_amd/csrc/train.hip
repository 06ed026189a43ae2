// train.hip — the training step's own kernels (reference train.py:26-67): the forward-diffusion
// perturbation, the loss and its gradient, gradient-norm clipping + Adam over flat parameter buffers, the step's Philox
// draws and keep masks, and the stand-alone bias gradient (colsum, behind dhw_op_colsum).  fp32 throughout.
// The rest of the training kernels lives under train/: the strided GEMM (sgemm_core.h, its instantiations sgemm_f32 /
// sgemm_bf16 / sgemm_group .hip and the planner sgemm_launch.hip), the element-wise / LayerNorm / softmax / pool /
// embedding passes (elementwise.hip) and the FiLM table (film_table.hip); dhw_train_convblock runs on those too.
#include <cstdlib>

#include "dhw_common.h"
#include <type_traits>
#include "dhw_kernels.h"
#include "heads_core.h"
#include "train/train_common.h"

using namespace dhw_train;

namespace {

// x_perturbed = sqrt(abar) x + sqrt(1 - abar) eps (train.py:41-43); alphas [B], x / eps [B, L, 2]
__global__ __launch_bounds__(256) void perturb_kernel(const float* x, const float* eps, const float* alphas, long n, int per_sample, float* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = alphas[i / per_sample];
  out[i] = sqrtf(a) * x[i] + sqrtf(1.0f - a) * eps[i];
}

// loss.py:5-37: score = mean_{b,l} sum_c (eps - pred)^2;  pen = mean_b( mean_l BCE(pen_pred, clamp(pen, 1e-7, 1-1e-7)) * abar_b ).
// One block per sample accumulates its two partial sums into out[1], out[2] (fp32 atomics, B adds each) and writes the
// gradients d loss / d pred [B,L,2], d loss / d pen_pred [B,L].  out[0] = out[1] + out[2] is formed by loss_finish.
__global__ __launch_bounds__(256) void loss_kernel(const float* eps, const float* pred, const float* pen, const float* pen_pred,
                                                    const float* alphas, int B, int L, float* out, float* d_pred, float* d_pen) {
  const int b = blockIdx.x;
  const float a = alphas[b];
  const float inv_bl = 1.0f / ((float)B * (float)L);
  float s = 0.f, q = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) {
    const long r = (long)b * L + l;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float d = eps[r * 2 + c] - pred[r * 2 + c];
      s += d * d;
      if (d_pred) d_pred[r * 2 + c] = -2.0f * d * inv_bl;
    }
    const float y = fminf(fmaxf(pen[r], 1e-7f), 1.0f - 1e-7f), pp = pen_pred[r];
    // torch's binary_cross_entropy clamps the logs at -100
    const float lp = fmaxf(logf(pp), -100.0f), lq = fmaxf(logf(1.0f - pp), -100.0f);
    q += -(y * lp + (1.0f - y) * lq);
    if (d_pen) d_pen[r] = (pp - y) / fmaxf(pp * (1.0f - pp), 1e-12f) * a * inv_bl;
  }
  __shared__ float rs[8], rq[8];
  for (int o = 32; o; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rq[threadIdx.x >> 6] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(out + 1, (rs[0] + rs[1] + rs[2] + rs[3]) * inv_bl);
    atomicAdd(out + 2, (rq[0] + rq[1] + rq[2] + rq[3]) * a * inv_bl);
  }
}
__global__ void loss_finish_kernel(float* out) { out[0] = out[1] + out[2]; }

// sum of squares of a flat buffer -> *out (atomic), for the global gradient norm (clip_grad.py:42-43, torch clip_grad_norm_)
// (16-byte loads, four independent partial sums per lane: 40 MB in ~10 us; the one-float-per-lane loop took 28)
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* g, long n, float* out) {
  float s = 0.f;
  const long stride = (long)gridDim.x * 256, t = (long)blockIdx.x * 256 + threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    const long n4 = n / 4;
    f32x4 a = (f32x4){0, 0, 0, 0}, b = a;
    long i = t;
    // (round 5: eight requests in flight per pass and 512 workgroups — 2048 workgroups x two requests took 32 us for the 40 MB gradient buffer:
    // five dependent round trips per thread and 2048 atomics on one address)
    for (; i + 7 * stride < n4; i += 8 * stride) {
      f32x4 u[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = g4[i + k * stride];
#pragma unroll
      for (int k = 0; k < 8; k += 2) { a += u[k] * u[k]; b += u[k + 1] * u[k + 1]; }
    }
    for (; i + stride < n4; i += 2 * stride) {
      const f32x4 u = g4[i], v = g4[i + stride];
      a += u * u;
      b += v * v;
    }
    if (i < n4) { const f32x4 u = g4[i]; a += u * u; }
    a += b;
    s = (a[0] + a[1]) + (a[2] + a[3]);
    for (long k = n4 * 4 + t; k < n; k += stride) s += g[k] * g[k];
  } else {
    for (long i = t; i < n; i += stride) s += g[i] * g[i];
  }
  __shared__ float r[4];
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, r[0] + r[1] + r[2] + r[3]);
}

// torch.optim.Adam (L2 weight decay folded into the gradient, bias-corrected moments) on a flat buffer, with the
// clip_grad_norm_ factor min(1, max_norm / (||g|| + 1e-6)) read from the device (sqnorm holds ||g||^2).
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float bc2, const float* sqnorm, float max_norm) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float clip = 1.0f;
  if (sqnorm) clip = fminf(1.0f, max_norm / (sqrtf(*sqnorm) + 1e-6f));
  const float gi = g[i] * clip + wd * p[i];
  const float mi = b1 * m[i] + (1.0f - b1) * gi;
  const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] -= lr / bc1 * mi / (sqrtf(vi) / sqrtf(bc2) + eps);
}

// The same update with its scalars read from device memory — hyper = {lr, beta1, beta2, eps, weight_decay, 1 - beta1^t,
// 1 - beta2^t, max_norm} — so that a captured hipGraph of the whole training step can be replayed with the step's own
// learning rate and bias corrections (the host rewrites the 8 floats before each replay).
// The scalars of one update as the kernels below read them, and the update of ONE element: the single statement of the arithmetic
// that adam_dev_kernel and adam_ema_kernel share, so that both contract the same expression into the same instructions.
struct AdamScalars { float lr, b1, b2, eps, wd, bc1, bc2, clip; };
__device__ __forceinline__ AdamScalars adam_scalars(const float* hyper, const float* sqnorm) {
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6], max_norm = hyper[7], gs = hyper[8];
  float clip = gs;   // (gs = 1 / world size behind a SUM all-reduce: the averaging costs no pass of its own; 1 otherwise)
  if (max_norm > 0.f) clip = gs * fminf(1.0f, max_norm / __builtin_fmaf(sqrtf(*sqnorm), gs, 1e-6f));   // (the FMA it has always been)
  return {lr, b1, b2, eps, wd, bc1, bc2, clip};
}
// Which products fuse into an FMA is written out rather than left to contraction: the compiler fused differently in the one-float and
// the four-float loop (m' came out as fma(b1, m, .) in the latter only).  What stands here is what adam_dev_kernel has always
// compiled to — the gradient term one FMA on the rounded wd * p, both moments as rounded products added — so its bits are unchanged.
__device__ __forceinline__ void adam_element(const AdamScalars& h, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const float gi = __builtin_fmaf(g, h.clip, h.wd * p);
  const float mi = h.b1 * m + (1.0f - h.b1) * gi;
  const float vi = h.b2 * v + (1.0f - h.b2) * gi * gi;
  m = mi;
  v = vi;
  p -= h.lr / h.bc1 * mi / (sqrtf(vi) / sqrtf(h.bc2) + h.eps);
}

__global__ __launch_bounds__(256) void adam_dev_kernel(float* p, const float* g, float* m, float* v, long n, const float* hyper, const float* sqnorm) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const AdamScalars h = adam_scalars(hyper, sqnorm);
  float pi = p[i], mi = m[i], vi = v[i];
  adam_element(h, g[i], pi, mi, vi);
  m[i] = mi;
  v[i] = vi;
  p[i] = pi;
}

// adam_dev_kernel's update and, in the same pass, the exponential moving average of the weights just written:
// ema' = fma(decay, ema, (1 - decay) p'), ema_hyper = {decay, 1 - decay} in DEVICE memory (both rounded by the host).  A streaming pass
// over nine streams (p, g, m, v, ema read; p, m, v, ema written): 16 bytes per lane and stream, at most ADAM_EMA_GRID workgroups
// striding over the buffer, the last n % 4 elements one per lane; `vec` = all five pointers are 16-byte aligned (the launcher
// tests them), else one float per lane in the same grid-stride loop.
constexpr unsigned ADAM_EMA_GRID = 2048;
__device__ __forceinline__ float ema_element(float decay, float omd, float e, float p_new) {
#pragma clang fp contract(off)
  return __builtin_fmaf(decay, e, omd * p_new);
}

__global__ __launch_bounds__(256) void adam_ema_kernel(float* p, const float* g, float* m, float* v, float* ema, long n, const float* hyper,
                                                        const float* ema_hyper, const float* sqnorm, int vec) {
  const AdamScalars h = adam_scalars(hyper, sqnorm);
  const float decay = ema_hyper[0], omd = ema_hyper[1];
  const long stride = (long)gridDim.x * 256, t = (long)blockIdx.x * 256 + threadIdx.x;
  long tail = 0;      // first element of the one-float-per-lane part
  if (vec) {
    const long n4 = n / 4;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    for (long i = t; i < n4; i += stride) {
      f32x4 pv = p4[i], mv = m4[i], vv = v4[i], ev = e4[i];
      const f32x4 gv = g4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pv[k], mk = mv[k], vk = vv[k];
        adam_element(h, gv[k], pk, mk, vk);
        pv[k] = pk; mv[k] = mk; vv[k] = vk;
        ev[k] = ema_element(decay, omd, ev[k], pk);
      }
      m4[i] = mv;
      v4[i] = vv;
      p4[i] = pv;
      e4[i] = ev;
    }
    tail = n4 * 4;
  }
  for (long i = tail + t; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_element(h, g[i], pi, mi, vi);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    ema[i] = ema_element(decay, omd, ema[i], pi);
  }
}

// The step's random draws on the device (train.py:39 eps = randn_like(x); text_style.py:97 Dropout(0.3) on the style
// features), from the sampler's counter-based Philox generator: rng = {seed, draw index} in DEVICE memory, so a captured
// graph draws fresh numbers at every replay once the host has bumped the index.  eps[b][l][:] = normal2(seed,
// sample = index * B + b, pos = l, iter = 0); the keep-mask uses iter = 1 and one Philox block per 4 elements.
__global__ __launch_bounds__(256) void train_draw_kernel(const uint64_t* rng, int B, int L, float* eps, long n_keep, int keep_per_sample, float p, float* keep) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const uint64_t seed = rng[0];
  const int64_t base = (int64_t)rng[1] * B;
  if (i < (long)B * L) {
    float z0, z1;
    normal2(seed, base + i / L, (int)(i % L), 0, z0, z1);
    eps[i * 2] = z0;
    eps[i * 2 + 1] = z1;
  }
  if (i * 4 < n_keep) {
    const long e = i * 4;
    const int64_t sample = base + e / keep_per_sample;
    uint32_t c0 = (uint32_t)sample, c1 = (uint32_t)((uint64_t)sample >> 32), c2 = (uint32_t)((e % keep_per_sample) / 4), c3 = 2u;   // iter + 1 = 2
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      philox_round(c0, c1, c2, c3, k0, k1);
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t c[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e + k < n_keep) keep[e + k] = ((float)(c[k] >> 8) + 0.5f) * (1.0f / 16777216.0f) >= p ? 1.0f : 0.0f;
  }
}

// A Dropout(p) keep-mask (1 = kept) over n elements, per_sample of them per batch sample, from the same generator:
// Philox block (sample = index * B + b, element / 4, site) — `site` >= 3 numbers the model's dropout sites (1 = eps, 2 = the
// style mask of train_draw_kernel), so every site of every update draws an independent mask.
__global__ __launch_bounds__(256) void keep_mask_kernel(const uint64_t* rng, uint32_t site, long n, int per_sample, float p, float* keep) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= n) return;
  const uint64_t seed = rng[0];
  const int64_t sample = (int64_t)rng[1] * (n / per_sample) + e / per_sample;
  uint32_t c0 = (uint32_t)sample, c1 = (uint32_t)((uint64_t)sample >> 32), c2 = (uint32_t)((e % per_sample) / 4), c3 = site;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint32_t c[4] = {c0, c1, c2, c3};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e + k < n) keep[e + k] = ((float)(c[k] >> 8) + 0.5f) * (1.0f / 16777216.0f) >= p ? 1.0f : 0.0f;
}

// db[c] += sum over all rows of dy[r][c]: block = 64 channels x 4 row groups over a chunk of rows, one atomic per (block, channel)
__global__ __launch_bounds__(256) void colsum_kernel(const float* dy, long rows, int C, int rows_per_block, float* db) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  float s = 0.f;
  if (c < C)
    for (long r = r0 + rg; r < r1; r += 4) s += dy[r * C + c];
  __shared__ float red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  if (rg == 0 && c < C) atomicAdd(db + c, red[threadIdx.x] + red[threadIdx.x + 64] + red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}

}  // namespace

hipError_t launch_perturb(const float* x, const float* eps, const float* alphas, int B, int L, float* out, hipStream_t st) {
  const long n = (long)B * L * 2;
  hipLaunchKernelGGL(perturb_kernel, dim3(nb(n)), dim3(256), 0, st, x, eps, alphas, n, L * 2, out);
  return hipGetLastError();
}
hipError_t launch_loss(const float* eps, const float* pred, const float* pen, const float* pen_pred, const float* alphas, int B, int L,
                       float* out3, float* d_pred, float* d_pen, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out3, 0, 3 * sizeof(float), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loss_kernel, dim3(B), dim3(256), 0, st, eps, pred, pen, pen_pred, alphas, B, L, out3, d_pred, d_pen);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1), 0, st, out3);
  return hipGetLastError();
}
hipError_t launch_sqnorm(const float* g, long n, float* out, hipStream_t st) {   // out must be zeroed by the caller (several buffers add up)
  hipLaunchKernelGGL(sqnorm_kernel, dim3(std::min<unsigned>(nb(n), 512u)), dim3(256), 0, st, g, n, out);
  return hipGetLastError();
}
hipError_t launch_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd, int step,
                       const float* sqnorm, float max_norm, hipStream_t st) {
  const float bc1 = 1.0f - powf(b1, (float)step), bc2 = 1.0f - powf(b2, (float)step);
  hipLaunchKernelGGL(adam_kernel, dim3(nb(n)), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2, sqnorm, max_norm);
  return hipGetLastError();
}
hipError_t launch_train_draw(const uint64_t* rng, int B, int L, float* eps, long n_keep, int keep_per_sample, float p, float* keep, hipStream_t st) {
  if (keep_per_sample % 4) return hipErrorInvalidValue;
  const long n = std::max((long)B * L, (n_keep + 3) / 4);
  hipLaunchKernelGGL(train_draw_kernel, dim3(nb(n)), dim3(256), 0, st, rng, B, L, eps, n_keep, keep_per_sample, p, keep);
  return hipGetLastError();
}
hipError_t launch_keep_mask(const uint64_t* rng, int site, long n, int per_sample, float p, float* keep, hipStream_t st) {
  if (per_sample % 4 || n % per_sample || site < 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(keep_mask_kernel, dim3(nb((n + 3) / 4)), dim3(256), 0, st, rng, (uint32_t)site, n, per_sample, p, keep);
  return hipGetLastError();
}
hipError_t launch_adam_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, const float* sqnorm, hipStream_t st) {
  hipLaunchKernelGGL(adam_dev_kernel, dim3(nb(n)), dim3(256), 0, st, p, g, m, v, n, hyper, sqnorm);
  return hipGetLastError();
}
hipError_t launch_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long n, const float* hyper, const float* ema_hyper,
                           const float* sqnorm, hipStream_t st) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                         reinterpret_cast<uintptr_t>(ema);
  const int vec = (bits & 15) == 0;
  // one lane per f32x4 (or per float in the scalar form); at least the n % 4 tail's one workgroup
  const unsigned grid = std::min<unsigned>(std::max(nb(vec ? n / 4 : n), 1u), ADAM_EMA_GRID);
  hipLaunchKernelGGL(adam_ema_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, ema, n, hyper, ema_hyper, sqnorm, vec);
  return hipGetLastError();
}
hipError_t launch_colsum(const float* dy, long rows, int C, float* db, hipStream_t st) {   // db zeroed by the caller
  const int rpb = 64;
  hipLaunchKernelGGL(colsum_kernel, dim3(nb(C, 64), nb(rows, rpb)), dim3(256), 0, st, dy, rows, C, rpb, db);
  return hipGetLastError();
}
