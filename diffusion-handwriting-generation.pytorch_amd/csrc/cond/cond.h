// cond.h — launchers of the replacement-conditioning kernels (include/dhw.h: dhw_sample_cond); shared by
// cond.hip, sampler/sample.cpp (the loop that launches them) and dhw_cond_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// iteration number the conditioning stream's k-th draw is keyed by: disjoint from -1 (x_T) and 0..T-1 (the sampler's own draws)
constexpr int COND_ITER0 = 1 << 30;

// What the three kernels share: one sub-batch [b0, b0 + Bs) of a conditioned call, every pointer already offset to its first row.
struct CondParams {
  float* x;                   // sampler state [rows, 2]
  const float* known;         // [rows, 3] = (dx, dy, pen)
  const unsigned char* keep;  // [rows], nonzero = kept, or null
  const int* lens;            // per-sample lengths of the sub-batch, or null
  long rows;                  // Bs * L
  int L;
  float ka, kb;               // sqrt(abar), sqrt(1 - abar) of the level the rows are noised to (computed on the host in fp32)
  // replace only: the conditioning draw of this iteration
  const float* z;             // cond_noise[k] of the sub-batch [rows, 2], or null -> the device generator
  const uint64_t* seed_ptr;   // [seed, first_sample]
  int sample_off;             // b0
  int iter;                   // COND_ITER0 + k
};

// rule 2: seeded rows (kept, or every valid row when `all`) become ka * known_xy + kb * x, x holding the start draw z
hipError_t launch_cond_start(const CondParams& p, int all, hipStream_t st);
// rule 3: kept rows become ka * known_xy + kb * zc
hipError_t launch_cond_replace(const CondParams& p, hipStream_t st);
// rule 4: kept rows of out3 [rows, 3] become known, all three columns
hipError_t launch_cond_finish(float* out3, const CondParams& p, hipStream_t st);
