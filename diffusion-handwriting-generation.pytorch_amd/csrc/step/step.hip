// step.hip — the small kernels of the eager samplers around the denoiser launches (include/dhw.h: dhw_ddim_sample,
// dhw_ddim_invert, dhw_ddim_update, dhw_guided_ddim_sample, dhw_guided_sample, dhw_guide_update, dhw_dpm_*; DESIGN.md §23, §33,
// §34, §40, §41).  ddim_start writes the first state; step_update moves a state from one noise level to the next along the denoiser's
// answer; its multistep kinds do so with the previous step's x0 estimate as well (second order) and keep the new estimate.
// Behind a guided call's forward over 2B rows that answer lies under the real condition in rows [0, B) of eps and under the
// guidance condition in rows [B, 2B): the guided instantiations combine the two per stroke row and write the new row to BOTH
// halves of the doubled state, so the next forward sees one x under two conditions.  Both kernels BRANCH on the lengths read at
// run time: a row at or past its sample's end is never read, whatever it holds, and is written as 0.  No atomics, no
// reductions: a row's result depends on that row alone.
#include "step.h"

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

// e = e_c + (w - 1) (e_c - e_u): the scalar w - 1, then a difference, a product and a sum per coordinate, each rounded on its own
// (plain operators under the pragma: cond.hip's cond_mix records why __fmul_rn does not do this).  w = 1: the product is a zero and
// e has e_c's value.  w = 0 is a SELECT of e_u: the arithmetic gives e_c - fl(e_c - e_u) there, which is e_u only where that
// difference is exact, and scale 0 is promised to be the guidance condition's own sample.
DHW_DEV float2 guide_combine(float2 ec, float2 eu, float w) {
#pragma clang fp contract(off)
  const float g = w - 1.0f;
  const float d0 = ec.x - eu.x, d1 = ec.y - eu.y;
  const float m0 = g * d0, m1 = g * d1;
  const float e0 = ec.x + m0, e1 = ec.y + m1;
  return w == 0.0f ? eu : make_float2(e0, e1);
}

// U(base, e; c0, c1, c2, c3) = fadd(fmul(c2, fdiv(fsub(base, fmul(c1, e)), c0)), fmul(c3, e)): plain operators under the
// pragma, so each of the five operations rounds on its own (cond.hip's cond_mix records why __fmul_rn does not do this); the
// division is the correctly rounded one (hipcc's default).  The one copy: guided and unguided DDIM steps both call it.
DHW_DEV float step_u(float base, float e, float c0, float c1, float c2, float c3) {
#pragma clang fp contract(off)
  const float m = c1 * e;
  const float d = base - m;
  const float x0 = d / c0;
  const float s = c2 * x0;
  const float n = c3 * e;
  return s + n;
}

// the ancestral steps in the operation order of heads_finish (heads_core.h), one rounding per operation
DHW_DEV float step_new(float x, float e, float z, float c0, float c1, float c2, bool add) {
#pragma clang fp contract(off)
  const float m = c0 * e;
  const float d = x - m;
  const float y = d / c1;
  const float n = z * c2;
  return add ? y + n : y;
}
DHW_DEV float step_standard(float x, float e, float z, float c0, float c1, float c2, float c3, bool add) {
#pragma clang fp contract(off)
  const float m = c3 * e;
  const float r = m / c0;
  const float d = x - r;
  const float y = c1 * d;
  const float n = c2 * z;
  return add ? y + n : y;
}

// the x0 estimate from (base, e) at level (c0, c1): the first three operations of step_u, the same roundings
DHW_DEV float step_x0(float base, float e, float c0, float c1) {
#pragma clang fp contract(off)
  const float m = c1 * e;
  const float d = base - m;
  return d / c0;
}

// the second-order multistep move from x0 and the previous step's x0 (hist): six operations, one rounding each
DHW_DEV float dpm_second(float x, float x0, float hist, float k0, float k1, float c4, float c5) {
#pragma clang fp contract(off)
  const float p = k0 * x0;
  const float q = k1 * hist;
  const float D = p - q;
  const float s = c4 * x;
  const float n = c5 * D;
  return s + n;
}

// One thread per stroke row of the B samples.  KIND and GUIDED are template arguments: the launcher switches, no lane does.
// !GUIDED takes eps[row] as it is (no combine: e + 0 * (e - e) would turn a -0 into +0 and an infinity into NaN) and touches
// nothing of a second half.  out3 (the last step of a sampling call) also gets the row with the denoiser's pen value.  A multistep
// kind leaves its x0 in hist, one half only, 0 at and past a length; its first-order step is step_u itself (the bits of
// dhw_ddim_update) and never reads hist.  A row reads its own base / hist entry before it writes it, so out may be base and hist is
// updated in place.
template <int KIND, bool GUIDED>
__global__ __launch_bounds__(256) void step_update_kernel(const StepParams p) {
  constexpr bool MULTISTEP = step_multistep(KIND);
  static_assert(GUIDED || KIND == STEP_DDIM || MULTISTEP, "the unguided ancestral steps are heads_finish's (heads_core.h)");
  const unsigned row = blockIdx.x * 256u + threadIdx.x;   // (halves * rows < 2^31, checked by the launcher: 32-bit index arithmetic)
  const unsigned rows = (unsigned)p.rows;
  if (row >= rows) return;
  const int b = (int)(row / (unsigned)p.L), pos = (int)(row - (unsigned)b * (unsigned)p.L);
  if (p.sigma && pos == 0) {
    p.sigma[b] = p.sigma_next;
    if (GUIDED) p.sigma[b + p.B] = p.sigma_next;
  }
  float2 x = make_float2(0.f, 0.f), x0 = make_float2(0.f, 0.f);
  float q = 0.f;
  if (pos < (p.lens ? p.lens[b] : p.L)) {
    const float2 base = reinterpret_cast<const float2*>(p.base)[row];
    float2 e = reinterpret_cast<const float2*>(p.eps)[row];
    if (GUIDED) e = guide_combine(e, reinterpret_cast<const float2*>(p.eps)[row + rows], p.scale[b]);
    if (MULTISTEP) {
      x0.x = step_x0(base.x, e.x, p.c0, p.c1);
      x0.y = step_x0(base.y, e.y, p.c0, p.c1);
    }
    if (KIND == STEP_DPM_SECOND) {
      const float2 h = reinterpret_cast<const float2*>(p.hist)[row];
      x.x = dpm_second(base.x, x0.x, h.x, p.k0, p.k1, p.c4, p.c5);
      x.y = dpm_second(base.y, x0.y, h.y, p.k0, p.k1, p.c4, p.c5);
    } else if (KIND == STEP_DDIM || KIND == STEP_DPM_FIRST) {
      x.x = step_u(base.x, e.x, p.c0, p.c1, p.c2, p.c3);
      x.y = step_u(base.y, e.y, p.c0, p.c1, p.c2, p.c3);
    } else {
      const bool add = p.add_noise != 0;   // (a kernel argument: uniform)
      float2 z = make_float2(0.f, 0.f);
      if (add) {
        if (p.z) z = reinterpret_cast<const float2*>(p.z)[row];
        else normal2(p.seed, p.first_sample + b, pos, p.iter, z.x, z.y);
      }
      if (KIND == STEP_NEW) {
        x.x = step_new(base.x, e.x, z.x, p.c0, p.c1, p.c2, add);
        x.y = step_new(base.y, e.y, z.y, p.c0, p.c1, p.c2, add);
      } else {
        x.x = step_standard(base.x, e.x, z.x, p.c0, p.c1, p.c2, p.c3, add);
        x.y = step_standard(base.y, e.y, z.y, p.c0, p.c1, p.c2, p.c3, add);
      }
    }
    if (p.out3) q = p.pen[row];
  }
  if (MULTISTEP) reinterpret_cast<float2*>(p.hist)[row] = x0;
  if (p.out) {
    reinterpret_cast<float2*>(p.out)[row] = x;
    if (GUIDED) reinterpret_cast<float2*>(p.out)[row + rows] = x;
  }
  if (p.out3) {
    float* o = p.out3 + (size_t)row * 3;
    o[0] = x.x;
    o[1] = x.y;
    o[2] = q;
  }
}

inline bool step_bad_shape(long rows, int B, int L, int halves) {
  return B < 1 || L < 1 || rows != (long)B * L || halves < 1 || halves > 2 || halves * rows > 0x7fffffffL;
}

}  // namespace

hipError_t launch_ddim_start(const DdimStartParams& p, hipStream_t st) {
  if (step_bad_shape(p.rows, p.B, p.L, 1) || !p.x || !p.sigma || (p.src && p.src_cols != 2 && p.src_cols != 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ddim_start_kernel, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_step_update(const StepParams& p, hipStream_t st) {
  const bool guided = p.halves == 2;
  if (step_bad_shape(p.rows, p.B, p.L, p.halves) || !p.base || !p.eps || (guided && !p.scale) || (!p.out && !p.out3) || (p.out3 && !p.pen) ||
      step_multistep(p.kind) != (p.hist != nullptr))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.rows + 255) / 256)), block(256);
#define STEP_LAUNCH(KIND, GUIDED) hipLaunchKernelGGL((step_update_kernel<KIND, GUIDED>), grid, block, 0, st, p)
  switch (p.kind * 2 + (guided ? 1 : 0)) {
    case STEP_DDIM * 2: STEP_LAUNCH(STEP_DDIM, false); break;
    case STEP_DDIM * 2 + 1: STEP_LAUNCH(STEP_DDIM, true); break;
    case STEP_NEW * 2 + 1: STEP_LAUNCH(STEP_NEW, true); break;
    case STEP_STANDARD * 2 + 1: STEP_LAUNCH(STEP_STANDARD, true); break;
    case STEP_DPM_FIRST * 2: STEP_LAUNCH(STEP_DPM_FIRST, false); break;
    case STEP_DPM_FIRST * 2 + 1: STEP_LAUNCH(STEP_DPM_FIRST, true); break;
    case STEP_DPM_SECOND * 2: STEP_LAUNCH(STEP_DPM_SECOND, false); break;
    case STEP_DPM_SECOND * 2 + 1: STEP_LAUNCH(STEP_DPM_SECOND, true); break;
    default: return hipErrorInvalidValue;   // (no such kind, or an unguided ancestral step)
  }
#undef STEP_LAUNCH
  return hipGetLastError();
}
