// guide.hip — the step of classifier-free guided sampling (include/dhw.h: dhw_guided_ddim_sample, dhw_guided_sample,
// dhw_guide_update).  One forward over 2B rows has left the denoiser's answer under the real condition in rows
// [0, B) of eps and under the guidance condition in rows [B, 2B); guide_update combines the two per stroke row, moves the state
// along the result and writes the new row to BOTH halves of the doubled state, so the next forward sees one x under two
// conditions.  Like ddim_update it BRANCHES on the lengths read at run time: a row at or past its sample's end is never read
// and is written as 0.  No atomics, no reductions: a row's result depends on that row alone.
#include "guide.h"

#include "../heads_core.h"

namespace {

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

// U of ddim.hip, five separately rounded operations (include/dhw.h)
DHW_DEV float guide_u(float base, float e, float c0, float c1, float c2, float c3) {
#pragma clang fp contract(off)
  const float m = c1 * e;
  const float d = base - m;
  const float x0 = d / c0;
  const float s = c2 * x0;
  const float n = c3 * e;
  return s + n;
}

// the ancestral steps in the operation order of heads_finish (heads_core.h), one rounding per operation
DHW_DEV float guide_new(float x, float e, float z, float c0, float c1, float c2, bool add) {
#pragma clang fp contract(off)
  const float m = c0 * e;
  const float d = x - m;
  const float y = d / c1;
  const float n = z * c2;
  return add ? y + n : y;
}
DHW_DEV float guide_standard(float x, float e, float z, float c0, float c1, float c2, float c3, bool add) {
#pragma clang fp contract(off)
  const float m = c3 * e;
  const float r = m / c0;
  const float d = x - r;
  const float y = c1 * d;
  const float n = c2 * z;
  return add ? y + n : y;
}

// One thread per stroke row of the B samples.  KIND is a template argument: the launcher switches, no lane does.
template <int KIND>
__global__ __launch_bounds__(256) void guide_update_kernel(const GuideParams p) {
  const unsigned row = blockIdx.x * 256u + threadIdx.x;   // (2 * rows < 2^31, checked by the launcher: 32-bit index arithmetic)
  const unsigned rows = (unsigned)p.rows;
  if (row >= rows) return;
  const int b = (int)(row / (unsigned)p.L), pos = (int)(row - (unsigned)b * (unsigned)p.L);
  if (p.sigma && pos == 0) {
    p.sigma[b] = p.sigma_next;
    p.sigma[b + p.B] = p.sigma_next;
  }
  float2 x = make_float2(0.f, 0.f);
  float q = 0.f;
  if (pos < (p.lens ? p.lens[b] : p.L)) {
    const float2 base = reinterpret_cast<const float2*>(p.x)[row];
    const float2 ec = reinterpret_cast<const float2*>(p.eps)[row], eu = reinterpret_cast<const float2*>(p.eps)[row + rows];
    const float2 e = guide_combine(ec, eu, p.scale[b]);
    if (KIND == GUIDE_DDIM) {
      x.x = guide_u(base.x, e.x, p.c0, p.c1, p.c2, p.c3);
      x.y = guide_u(base.y, e.y, p.c0, p.c1, p.c2, p.c3);
    } else {
      const bool add = p.add_noise != 0;   // (a kernel argument: uniform)
      float2 z = make_float2(0.f, 0.f);
      if (add) {
        if (p.z) z = reinterpret_cast<const float2*>(p.z)[row];
        else normal2(p.seed, p.first_sample + b, pos, p.iter, z.x, z.y);
      }
      if (KIND == GUIDE_NEW) {
        x.x = guide_new(base.x, e.x, z.x, p.c0, p.c1, p.c2, add);
        x.y = guide_new(base.y, e.y, z.y, p.c0, p.c1, p.c2, add);
      } else {
        x.x = guide_standard(base.x, e.x, z.x, p.c0, p.c1, p.c2, p.c3, add);
        x.y = guide_standard(base.y, e.y, z.y, p.c0, p.c1, p.c2, p.c3, add);
      }
    }
    if (p.out3) q = p.pen[row];
  }
  if (p.out) {
    reinterpret_cast<float2*>(p.out)[row] = x;
    reinterpret_cast<float2*>(p.out)[row + rows] = x;
  }
  if (p.out3) {
    float* o = p.out3 + (size_t)row * 3;
    o[0] = x.x;
    o[1] = x.y;
    o[2] = q;
  }
}

}  // namespace

hipError_t launch_guide_update(const GuideParams& p, hipStream_t st) {
  if (p.B < 1 || p.L < 1 || p.rows != (long)p.B * p.L || 2 * p.rows > 0x7fffffffL) return hipErrorInvalidValue;
  if (!p.x || !p.eps || !p.scale || (!p.out && !p.out3) || (p.out3 && !p.pen)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.rows + 255) / 256)), block(256);
  switch (p.kind) {
    case GUIDE_DDIM: hipLaunchKernelGGL(guide_update_kernel<GUIDE_DDIM>, grid, block, 0, st, p); break;
    case GUIDE_NEW: hipLaunchKernelGGL(guide_update_kernel<GUIDE_NEW>, grid, block, 0, st, p); break;
    case GUIDE_STANDARD: hipLaunchKernelGGL(guide_update_kernel<GUIDE_STANDARD>, grid, block, 0, st, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
