// step.h — launchers of the eager samplers' small kernels (include/dhw.h: dhw_ddim_sample, dhw_ddim_invert, dhw_ddim_update,
// dhw_guided_ddim_sample, dhw_guided_sample, dhw_guide_update, dhw_dpm_update, dhw_dpm_sample, dhw_guided_dpm_sample; DESIGN.md
// §23, §33, §34, §40, §41); shared by step.hip and dhw_step_api.cpp (the loops that launch them around the denoiser).
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

// The update a step makes.  0 / 1 / 2 are GuideKind's numbers (dhw_guide_update's `kind`); the two behind them are the multistep
// solver's first- and second-order step (include/dhw.h dhw_dpm_update), internal: dhw_step_api.cpp translates
// solver_host.h's DpmKind, the row format of dhw_dpm_coefs, into them.
enum StepKind { STEP_DDIM = GUIDE_DDIM, STEP_NEW = GUIDE_NEW, STEP_STANDARD = GUIDE_STANDARD, STEP_DPM_FIRST = 3, STEP_DPM_SECOND = 4 };
static_assert(STEP_DDIM == 0 && STEP_NEW == 1 && STEP_STANDARD == 2 && STEP_DPM_FIRST == GUIDE_STANDARD + 1,
              "the public kinds keep GuideKind's numbers; the internal ones follow them");
constexpr bool step_multistep(int kind) { return kind == STEP_DPM_FIRST || kind == STEP_DPM_SECOND; }

// One step per stroke row r = b*L + p of the B samples.  halves = 1: the update `kind` (not an ancestral one) of (base[r], eps[r]).
// halves = 2, a guided step behind a forward of 2B rows: e = combine(eps[r], eps[r + rows], scale[b]), then the update `kind` of
// (base[r], e), written to BOTH halves of the doubled state.  A multistep kind also writes hist[r] = x0 = (base - c1 e) / c0;
// STEP_DPM_FIRST is otherwise STEP_DDIM (U's bits), STEP_DPM_SECOND the nine operations on (base, e, hist[r]).
// ONE block for every kind: the multistep fields are APPENDED, so no field of §34's block moved and the kernels
// that do not read them load what they loaded before (§34 and §40 feared a wider block; that holds for an inserted field only).
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
  int kind;               // StepKind
  float c0, c1, c2, c3;   // computed on the host in fp32 (ddim_host.h / guide_host.h / solver_host.h), passed by value
  int add_noise;          // ancestral kinds: the noise term is added
  uint64_t seed;          // the generator's key and counters, as normal2 takes them
  int64_t first_sample;
  int iter;
  float* out;             // [halves*rows, 2]: the new row goes to r (and to r + rows); may be `base`: a thread reads its own row
                          // before it writes it; or null with out3
  float* out3;            // [rows, 3] = (x, pen): the last step of a sampling call, or null
  float* sigma;           // [halves*B]: b (and b + B) receive sigma_next for the next forward, or null
  float sigma_next;
  // the multistep kinds only, behind everything else
  float* hist;            // [rows, 2], one half only: read by a second-order step (its own row, before it is written), written by
                          // every multistep step; null for the other kinds
  float k0, k1, c4, c5;   // STEP_DPM_SECOND only (solver_host.h)
};

hipError_t launch_ddim_start(const DdimStartParams& p, hipStream_t st);
hipError_t launch_step_update(const StepParams& p, hipStream_t st);
