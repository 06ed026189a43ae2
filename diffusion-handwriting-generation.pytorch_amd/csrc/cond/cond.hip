// cond.hip — replacement conditioning of the reverse process (include/dhw.h: dhw_sample_cond): the state of
// chosen stroke rows is set to the known strokes noised to the current level — once in front of the loop (start), after every
// scheduler step (replace), and in the [B,L,3] output (finish).  One thread per stroke row, float2 access to the state.  The
// kernels BRANCH on keep / lengths read at run time: a row that is not seeded is never read from `known`, whatever it holds,
// and one captured graph serves every mask of a shape.
#include "cond.h"

#include "../heads_core.h"

namespace {

// the row's position is valid (inside its sample's length)
DHW_DEV bool cond_valid(const CondParams& p, long row) { return !p.lens || (int)(row % p.L) < p.lens[row / p.L]; }

// Two products and one sum, each rounded to nearest on its own: fadd(fmul(ka, known), fmul(kb, z)).  Written with plain
// operators under the pragma: to this compiler __fmul_rn / __fadd_rn ARE plain * and +, compiled inside their header, where
// HIP's default -ffp-contract=fast still fuses a product into the sum (v_pk_fma_f32 in the ISA) whatever the caller asks for.
DHW_DEV float2 cond_mix(const CondParams& p, long row, float2 z) {
#pragma clang fp contract(off)
  const float k0 = p.known[row * 3], k1 = p.known[row * 3 + 1];
  const float a0 = p.ka * k0, a1 = p.ka * k1, b0 = p.kb * z.x, b1 = p.kb * z.y;
  return make_float2(a0 + b0, a1 + b1);
}

__global__ __launch_bounds__(256) void cond_start_kernel(const CondParams p, int all) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= p.rows || !cond_valid(p, row)) return;
  if (!all && !(p.keep && p.keep[row])) return;
  float2* x = reinterpret_cast<float2*>(p.x);
  x[row] = cond_mix(p, row, x[row]);
}

__global__ __launch_bounds__(256) void cond_replace_kernel(const CondParams p) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= p.rows || !cond_valid(p, row) || !p.keep[row]) return;
  float2 z;
  if (p.z) z = reinterpret_cast<const float2*>(p.z)[row];
  else normal2(p.seed_ptr[0], (int64_t)p.seed_ptr[1] + p.sample_off + row / p.L, (int)(row % p.L), p.iter, z.x, z.y);
  reinterpret_cast<float2*>(p.x)[row] = cond_mix(p, row, z);
}

__global__ __launch_bounds__(256) void cond_finish_kernel(float* out3, const CondParams p) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= p.rows || !cond_valid(p, row) || !p.keep[row]) return;
  for (int c = 0; c < 3; ++c) out3[row * 3 + c] = p.known[row * 3 + c];
}

inline unsigned cond_blocks(long rows) { return (unsigned)((rows + 255) / 256); }
inline bool cond_bad(const CondParams& p) { return !p.known || p.rows < 1 || p.L < 1; }

}  // namespace

hipError_t launch_cond_start(const CondParams& p, int all, hipStream_t st) {
  if (cond_bad(p) || !p.x) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cond_start_kernel, dim3(cond_blocks(p.rows)), dim3(256), 0, st, p, all);
  return hipGetLastError();
}
hipError_t launch_cond_replace(const CondParams& p, hipStream_t st) {
  if (cond_bad(p) || !p.x || !p.keep || (!p.z && !p.seed_ptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cond_replace_kernel, dim3(cond_blocks(p.rows)), dim3(256), 0, st, p);
  return hipGetLastError();
}
hipError_t launch_cond_finish(float* out3, const CondParams& p, hipStream_t st) {
  if (cond_bad(p) || !out3 || !p.keep) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cond_finish_kernel, dim3(cond_blocks(p.rows)), dim3(256), 0, st, out3, p);
  return hipGetLastError();
}
