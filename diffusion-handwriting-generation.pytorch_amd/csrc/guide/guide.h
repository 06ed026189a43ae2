// guide.h — launcher of the guided step kernel (include/dhw.h: dhw_guided_ddim_sample, dhw_guided_sample, dhw_guide_update;
// DESIGN.md §33); shared by guide.hip and dhw_guide_api.cpp (the loops that launch it behind the 2B-row forward).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "guide_host.h"

// One guided step per stroke row r = b*L + p of the B samples: e = combine(eps[r], eps[r + rows], scale[b]), then the update
// `kind` of (x[r], e), written to BOTH halves of the doubled state.
struct GuideParams {
  const float* x;         // the state; rows [0, rows) are read
  const float* eps;       // [2*rows, 2]: the conditional half, then the guidance half
  const float* pen;       // [rows] of the conditional half (read with out3 only)
  const int* lens;        // per-sample lengths (device, B entries: both halves), or null
  const float* scale;     // [B] (device)
  const float* z;         // [rows, 2] the iteration's noise, or null -> the device generator (ancestral kinds with add_noise)
  long rows;              // B * L
  int B, L;
  int kind;               // GuideKind
  float c0, c1, c2, c3;   // computed on the host in fp32 (ddim_host.h / guide_host.h), passed by value
  int add_noise;          // ancestral kinds: the noise term is added
  uint64_t seed;          // the generator's key and counters, as normal2 takes them
  int64_t first_sample;
  int iter;
  float* out;             // [2*rows, 2]: the new row goes to r and to r + rows (may be `x`), or null with out3
  float* out3;            // [rows, 3] = (x, pen of the conditional row), or null
  float* sigma;           // [2*B]: b and b + B receive sigma_next, or null
  float sigma_next;
};

hipError_t launch_guide_update(const GuideParams& p, hipStream_t st);
