// ddim_host.h — the host arithmetic of dhw_ddim_sample / dhw_ddim_invert (include/dhw.h) that needs neither a handle nor a
// device: the checks of T, S, levels (over host/levels.h) and iters, and the table of per-step coefficients.  Plain C++
// (tests/cpp/ddim_host_check.cpp compiles it alone).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../host/levels.h"

constexpr int DDIM_MAX_ITERS = 8;      // fixed-point iterations per inversion step

// the level of step j: A = sqrtf(a_j), B = sqrtf(1 - a_j); entry S is the clean end (1, 0)
struct DdimCoef {
  float A, B;
};

// The checks the ddim entries add to the forward entry's: check_levels with their own count name, strictly decreasing levels.
inline int ddim_check_levels(int T, const int32_t* levels, int S, char* msg, size_t msg_len) { return check_levels(T, levels, S, "S", true, msg, msg_len); }

inline int ddim_check_iters(int iters, char* msg, size_t msg_len) {
  if (iters < 1 || iters > DDIM_MAX_ITERS) { snprintf(msg, msg_len, "iters = %d must lie in [1, %d]", iters, DDIM_MAX_ITERS); return -1; }
  return 0;
}

// levels (checked) -> S + 1 coefficient pairs; abar holds the T entries dhw_schedule gives.  fp32 throughout.
inline std::vector<DdimCoef> ddim_coef_table(const float* abar, const int32_t* levels, int S) {
  std::vector<DdimCoef> t((size_t)S + 1);
  for (int j = 0; j < S; ++j) {
    const float a = abar[levels[j]];
    t[(size_t)j] = DdimCoef{sqrtf(a), sqrtf(1.0f - a)};
  }
  t[(size_t)S] = DdimCoef{1.0f, 0.0f};
  return t;
}
