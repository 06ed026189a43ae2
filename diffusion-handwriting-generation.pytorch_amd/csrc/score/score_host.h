// score_host.h — the host arithmetic of dhw_score (include/dhw.h) that needs neither a handle nor a device: the checks of T,
// K and levels (over host/levels.h) and the table of per-level coefficients.  Plain C++ (tests/cpp/score_host_check.cpp compiles it alone).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../host/levels.h"

// iteration number the scoring draw of schedule index i is keyed by: disjoint from the sampler's (-1 .. T-1) and from the
// conditioning stream's (2^30 + k); T <= MAX_T keeps SCORE_ITER0 + i below 2^30
constexpr int SCORE_ITER0 = 1 << 29;

// one noise level of a dhw_score call
struct ScoreLevel {
  float ka, kb;   // sqrtf(abar[i]), sqrtf(1 - abar[i])
  float abar;     // abar[i]: the weight of the pen term
  int iter;       // SCORE_ITER0 + i
};

// The checks dhw_score adds to the forward entry's: check_levels with its own count name, any order, duplicates allowed.
inline int score_check_levels(int T, const int32_t* levels, int K, char* msg, size_t msg_len) { return check_levels(T, levels, K, "K", false, msg, msg_len); }

// levels (checked) -> coefficients; abar holds the T entries dhw_schedule gives.  fp32 throughout.
inline std::vector<ScoreLevel> score_level_table(const float* abar, const int32_t* levels, int K) {
  std::vector<ScoreLevel> t((size_t)K);
  for (int k = 0; k < K; ++k) {
    const float a = abar[levels[k]];
    t[(size_t)k] = ScoreLevel{sqrtf(a), sqrtf(1.0f - a), a, SCORE_ITER0 + (int)levels[k]};
  }
  return t;
}
