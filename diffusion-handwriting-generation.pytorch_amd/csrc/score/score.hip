// score.hip — the denoising objective of given strokes at one noise level (include/dhw.h: dhw_score), around
// the denoiser launches: score_perturb noises the strokes to the level (and keeps the draw), score_reduce turns the
// denoiser's answer into the two per-sample means.  Both BRANCH on the lengths read at run time: a row at or past its
// sample's end is never read from `strokes` or `noise`, whatever it holds.
#include "score.h"

#include "../heads_core.h"

namespace {

DHW_DEV int score_len(const ScoreParams& p, int b) { return p.lens ? p.lens[b] : p.L; }

// One thread per stroke row: z = the given draw or the generator's, x_t = fadd(fmul(ka, x0), fmul(kb, z)).  Plain operators
// under the pragma: each product and the sum round on their own (cond.hip's cond_mix records why __fmul_rn does not do this).
__global__ __launch_bounds__(256) void score_perturb_kernel(const ScoreParams p) {
#pragma clang fp contract(off)
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= p.rows) return;
  const int b = (int)(row / p.L), pos = (int)(row % p.L);
  if (pos == 0) p.sigma[b] = p.lv.ka;
  if (pos >= score_len(p, b)) return;
  float2 z;
  if (p.noise) z = reinterpret_cast<const float2*>(p.noise)[row];
  else normal2(p.seed, p.first_sample + b, pos, p.lv.iter, z.x, z.y);
  const float x0 = p.strokes[row * 3], x1 = p.strokes[row * 3 + 1];
  const float a0 = p.lv.ka * x0, a1 = p.lv.ka * x1, b0 = p.lv.kb * z.x, b1 = p.lv.kb * z.y;
  reinterpret_cast<float2*>(p.xt)[row] = make_float2(a0 + b0, a1 + b1);
  reinterpret_cast<float2*>(p.z)[row] = z;
}

// the sum over the 64 lanes of a wave, in every lane, by a butterfly of fixed shape
DHW_DEV float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One 256-thread workgroup per sample.  Thread t sums rows t, t + 256, ... in that order; the four waves reduce by
// butterfly, exchange their sums through LDS, and thread 0 adds them as ((w0 + w1) + w2) + w3: the order depends on the
// sample's own length alone, so a row of a batch and the same sample scored alone agree bit for bit.
__global__ __launch_bounds__(256) void score_reduce_kernel(const ScoreParams p) {
#pragma clang fp contract(off)
  __shared__ float part[2][4];
  const int b = blockIdx.x, n = score_len(p, b), tid = threadIdx.x;
  const long row0 = (long)b * p.L;
  float se = 0.f, sp = 0.f;
  for (int pos = tid; pos < n; pos += 256) {
    const long row = row0 + pos;
    const float2 z = reinterpret_cast<const float2*>(p.z)[row], e = reinterpret_cast<const float2*>(p.eps)[row];
    const float d0 = z.x - e.x, d1 = z.y - e.y;
    se += d0 * d0 + d1 * d1;
    const float q = p.pen[row];
    const float t = fminf(fmaxf(p.strokes[row * 3 + 2], 1e-7f), 1.0f - 1e-7f);
    sp += -(t * fmaxf(logf(q), -100.f) + (1.0f - t) * fmaxf(logf(1.0f - q), -100.f));
  }
  se = wave_sum(se);
  sp = wave_sum(sp);
  if ((tid & 63) == 0) { part[0][tid >> 6] = se; part[1][tid >> 6] = sp; }
  __syncthreads();
  if (tid == 0) {
    const float e = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    const float c = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    reinterpret_cast<float2*>(p.out)[b] = make_float2(e / (float)n, p.lv.abar * (c / (float)n));
  }
}

inline bool score_bad(const ScoreParams& p) { return !p.strokes || !p.z || p.B < 1 || p.L < 1 || p.rows != (long)p.B * p.L; }

}  // namespace

hipError_t launch_score_perturb(const ScoreParams& p, hipStream_t st) {
  if (score_bad(p) || !p.xt || !p.sigma) return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_perturb_kernel, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}
hipError_t launch_score_reduce(const ScoreParams& p, hipStream_t st) {
  if (score_bad(p) || !p.eps || !p.pen || !p.out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)p.B), dim3(256), 0, st, p);
  return hipGetLastError();
}
