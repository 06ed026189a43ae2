// step.h — launchers of the eager samplers' small kernels (include/dhw.h: dhw_ddim_sample, dhw_ddim_invert, dhw_ddim_update,
// dhw_guided_ddim_sample, dhw_guided_sample, dhw_guide_update, dhw_dpm_update, dhw_dpm_sample, dhw_guided_dpm_sample; DESIGN.md
// §23, §33, §34, §40); shared by step.hip and dhw_step_api.cpp (the loops that launch them around the denoiser).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../guide/guide_host.h"

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

// One step per stroke row r = b*L + p of the B samples.  halves = 1: the update `kind` (GUIDE_DDIM only) of (base[r], eps[r]).
// halves = 2, a guided step behind a forward of 2B rows: e = combine(eps[r], eps[r + rows], scale[b]), then the update `kind` of
// (base[r], e), written to BOTH halves of the doubled state.
struct StepParams {
  const float* base;      // the state; rows [0, rows) are read
  const float* eps;       // [halves*rows, 2]: the conditional half, then (halves = 2) the guidance half
  const float* pen;       // [rows], the denoiser's pen output of the conditional half (read with out3 only)
  const int* lens;        // per-sample lengths (device, B entries: both halves), or null
  const float* scale;     // [B] (device); halves = 2 only
  const float* z;         // [rows, 2] the iteration's noise, or null -> the device generator (ancestral kinds with add_noise)
  long rows;              // B * L
  int B, L;
  int halves;             // 1 or 2
  int kind;               // GuideKind
  float c0, c1, c2, c3;   // computed on the host in fp32 (ddim_host.h / guide_host.h), passed by value
  int add_noise;          // ancestral kinds: the noise term is added
  uint64_t seed;          // the generator's key and counters, as normal2 takes them
  int64_t first_sample;
  int iter;
  float* out;             // [halves*rows, 2]: the new row goes to r (and to r + rows); may be `base`: a thread reads its own row
                          // before it writes it; or null with out3
  float* out3;            // [rows, 3] = (x, pen): the last step of a sampling call, or null
  float* sigma;           // [halves*B]: b (and b + B) receive sigma_next for the next forward, or null
  float sigma_next;
};

// One step of the second-order multistep solver (include/dhw.h dhw_dpm_update) per stroke row r = b*L + p of the B
// samples; its own block: StepParams keeps its size (§34: a wider argument block changes the existing kernels' scalar loads).
// second = 0: x' = U(base, e; c0, c1, c2, c3), step_update's bits.  second = 1: the nine operations on (base, e, hist[r]).  Both
// write hist[r] = x0 = (base - c1 e) / c0.  halves = 2: e = combine(eps[r], eps[r + rows], scale[b]), x' goes to both halves.
struct DpmParams {
  const float* base;      // the state; rows [0, rows) are read
  const float* eps;       // [halves*rows, 2]
  const float* pen;       // [rows] (read with out3 only)
  const int* lens;        // per-sample lengths (device, B entries), or null
  const float* scale;     // [B] (device); halves = 2 only
  float* hist;            // [rows, 2], one half only: read by a second-order step (its own row, before it is written), written by every step
  long rows;              // B * L
  int B, L;
  int halves;             // 1 or 2
  int second;             // 0: first order, 1: second order
  float c0, c1, c2, c3;   // A_j, B_j, A_{j+1}, B_{j+1}
  float k0, k1, c4, c5;   // second order only (solver_host.h)
  float* out;             // [halves*rows, 2] (may be `base`), or null with out3
  float* out3;            // [rows, 3] = (x', pen): the last step of a sampling call, or null
  float* sigma;           // [halves*B], or null
  float sigma_next;
};

hipError_t launch_ddim_start(const DdimStartParams& p, hipStream_t st);
hipError_t launch_step_update(const StepParams& p, hipStream_t st);
hipError_t launch_dpm_update(const DpmParams& p, hipStream_t st);
