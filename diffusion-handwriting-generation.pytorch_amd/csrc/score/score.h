// score.h — launchers of the scoring kernels (include/dhw.h: dhw_score); shared by score.hip and
// dhw_score_api.cpp (the loop over noise levels that launches them around the denoiser).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_host.h"

// What the two kernels of one noise level share: every pointer already offset to the level's first row.
struct ScoreParams {
  const float* strokes;   // [rows, 3] = (dx, dy, pen), the caller's
  const int* lens;        // per-sample lengths (device), or null
  long rows;              // B * L
  int B, L;
  ScoreLevel lv;          // the level's coefficients (score_host.h), computed on the host in fp32
  // perturb only
  const float* noise;     // noise[k] [rows, 2], or null -> the device generator
  uint64_t seed;
  int64_t first_sample;
  float* xt;              // out: x_t [rows, 2]
  float* sigma;           // out: [B], sqrt(abar) for every sample
  // perturb writes, reduce reads
  float* z;               // [rows, 2]
  // reduce only
  const float* eps;       // eps_hat [rows, 2]
  const float* pen;       // pen_hat [rows]
  float* out;             // out[k] [B, 2]
};

// rules 1, 2, 5: z (given or drawn) and x_t = ka * x0 + kb * z of every valid row; sigma[b] = ka
hipError_t launch_score_perturb(const ScoreParams& p, hipStream_t st);
// rule 4: out[b] = (mean squared eps error, abar * mean pen cross-entropy) over the valid rows of sample b
hipError_t launch_score_reduce(const ScoreParams& p, hipStream_t st);
