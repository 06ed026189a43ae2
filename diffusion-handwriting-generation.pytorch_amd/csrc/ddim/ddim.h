// ddim.h — launchers of the deterministic-sampling kernels (include/dhw.h: dhw_ddim_sample, dhw_ddim_invert,
// dhw_ddim_update); shared by ddim.hip and dhw_ddim_api.cpp (the loops that launch them around the denoiser).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddim_host.h"

// The start of a call: x = the given rows (a latent [rows, 2] or strokes [rows, 3], first two columns) or the generator's draw.
struct DdimStartParams {
  const float* src;       // given rows, or null -> the device generator
  int src_cols;           // 2 (latent: float2 loads) or 3 (strokes: the pen column is not read)
  const int* lens;        // per-sample lengths (device), or null
  long rows;              // B * L
  int B, L;
  uint64_t seed;
  int64_t first_sample;
  float* x;               // out: [rows, 2], 0 at and past lens[b]
  float* copy;            // out: the same values once more (latent_out), or null
  float* sigma;           // out: [B], the first forward's sigma for every sample
  float sigma0;
};

// One update U(base, e; c0, c1, c2, c3) per stroke row and coordinate (include/dhw.h).
struct DdimParams {
  const float* base;      // [rows, 2]
  const float* eps;       // [rows, 2]
  const int* lens;        // per-sample lengths (device), or null
  long rows;              // B * L
  int B, L;
  float c0, c1, c2, c3;   // computed on the host in fp32 (ddim_host.h), passed by value
  float* out;             // [rows, 2] (may be `base`: a thread reads its own row before it writes it), or null with out3
  // the last step of a sampling call
  const float* pen;       // [rows], the denoiser's pen output
  float* out3;            // [rows, 3] = (x, pen), or null
  // the next forward
  float* sigma;           // [B] or null
  float sigma_next;
};

hipError_t launch_ddim_start(const DdimStartParams& p, hipStream_t st);
hipError_t launch_ddim_update(const DdimParams& p, hipStream_t st);
