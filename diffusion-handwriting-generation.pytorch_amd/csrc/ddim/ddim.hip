// ddim.hip — deterministic (DDIM, eta = 0) sampling and inversion around the denoiser launches (include/dhw.h:
// dhw_ddim_sample, dhw_ddim_invert, dhw_ddim_update).  ddim_start writes the first state, ddim_update moves a
// state from one noise level to another along the denoiser's answer.  Both BRANCH on the lengths read at run time: a row at
// or past its sample's end is never read, whatever it holds, and is written as 0.  No atomics, no reductions: a row's result
// depends on that row alone.
#include "ddim.h"

#include "../heads_core.h"

namespace {

// One thread per stroke row: x = the given row (a float2 of a latent, or the first two columns of a stroke row) or the
// generator's draw for (seed, first_sample + b, pos, iter = -1), the x_T of dhw_sample.
__global__ __launch_bounds__(256) void ddim_start_kernel(const DdimStartParams p) {
  const unsigned row = blockIdx.x * 256u + threadIdx.x;   // (rows < 2^31, checked by the launcher: 32-bit index arithmetic)
  if (row >= (unsigned)p.rows) return;
  const int b = (int)(row / (unsigned)p.L), pos = (int)(row - (unsigned)b * (unsigned)p.L);
  if (pos == 0) p.sigma[b] = p.sigma0;
  float2 x = make_float2(0.f, 0.f);
  if (pos < (p.lens ? p.lens[b] : p.L)) {
    if (!p.src) normal2(p.seed, p.first_sample + b, pos, -1, x.x, x.y);
    else if (p.src_cols == 2) x = reinterpret_cast<const float2*>(p.src)[row];
    else x = make_float2(p.src[(size_t)row * 3], p.src[(size_t)row * 3 + 1]);
  }
  reinterpret_cast<float2*>(p.x)[row] = x;
  if (p.copy) reinterpret_cast<float2*>(p.copy)[row] = x;
}

// U(base, e; c0, c1, c2, c3) = fadd(fmul(c2, fdiv(fsub(base, fmul(c1, e)), c0)), fmul(c3, e)): plain operators under the
// pragma, so each of the five operations rounds on its own (cond.hip's cond_mix records why __fmul_rn does not do this); the
// division is the correctly rounded one (hipcc's default).
DHW_DEV float ddim_u(float base, float e, float c0, float c1, float c2, float c3) {
#pragma clang fp contract(off)
  const float m = c1 * e;
  const float d = base - m;
  const float x0 = d / c0;
  const float s = c2 * x0;
  const float n = c3 * e;
  return s + n;
}

// One thread per stroke row.  out3 (the last step of a sampling call) also gets the row with the denoiser's pen value.
__global__ __launch_bounds__(256) void ddim_update_kernel(const DdimParams p) {
  const unsigned row = blockIdx.x * 256u + threadIdx.x;   // (rows < 2^31, checked by the launcher: 32-bit index arithmetic)
  if (row >= (unsigned)p.rows) return;
  const int b = (int)(row / (unsigned)p.L), pos = (int)(row - (unsigned)b * (unsigned)p.L);
  if (p.sigma && pos == 0) p.sigma[b] = p.sigma_next;
  float2 x = make_float2(0.f, 0.f);
  float q = 0.f;
  if (pos < (p.lens ? p.lens[b] : p.L)) {
    const float2 base = reinterpret_cast<const float2*>(p.base)[row], e = reinterpret_cast<const float2*>(p.eps)[row];
    x.x = ddim_u(base.x, e.x, p.c0, p.c1, p.c2, p.c3);
    x.y = ddim_u(base.y, e.y, p.c0, p.c1, p.c2, p.c3);
    if (p.out3) q = p.pen[row];
  }
  if (p.out) reinterpret_cast<float2*>(p.out)[row] = x;
  if (p.out3) {
    float* o = p.out3 + (size_t)row * 3;
    o[0] = x.x;
    o[1] = x.y;
    o[2] = q;
  }
}

inline bool ddim_bad_shape(long rows, int B, int L) { return B < 1 || L < 1 || rows != (long)B * L || rows > 0x7fffffffL; }

}  // namespace

hipError_t launch_ddim_start(const DdimStartParams& p, hipStream_t st) {
  if (ddim_bad_shape(p.rows, p.B, p.L) || !p.x || !p.sigma || (p.src && p.src_cols != 2 && p.src_cols != 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ddim_start_kernel, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}
hipError_t launch_ddim_update(const DdimParams& p, hipStream_t st) {
  if (ddim_bad_shape(p.rows, p.B, p.L) || !p.base || !p.eps || (!p.out && !p.out3) || (p.out3 && !p.pen)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ddim_update_kernel, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}
