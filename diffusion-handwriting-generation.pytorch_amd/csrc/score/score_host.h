// score_host.h — the host arithmetic of dhw_score (include/dhw.h) that needs neither a handle nor a device: the checks of T,
// K and levels, and the table of per-level coefficients.  Plain C++ (tests/cpp/score_host_check.cpp compiles it alone).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

// iteration number the scoring draw of schedule index i is keyed by: disjoint from the sampler's (-1 .. T-1) and from the
// conditioning stream's (2^30 + k)
constexpr int SCORE_ITER0 = 1 << 29;

// one noise level of a dhw_score call
struct ScoreLevel {
  float ka, kb;   // sqrtf(abar[i]), sqrtf(1 - abar[i])
  float abar;     // abar[i]: the weight of the pen term
  int iter;       // SCORE_ITER0 + i
};

// The checks dhw_score adds to the forward entry's: 0 on success, else -1 with the offending argument named in msg.
inline int score_check_levels(int T, const int32_t* levels, int K, char* msg, size_t msg_len) {
  if (T < 1 || T > SCORE_ITER0) { snprintf(msg, msg_len, "T = %d must lie in [1, 2^29]", T); return -1; }
  if (K < 1 || K > T) { snprintf(msg, msg_len, "K = %d must lie in [1, T = %d]", K, T); return -1; }
  if (!levels) { snprintf(msg, msg_len, "levels is NULL (K = %d entries expected)", K); return -1; }
  for (int k = 0; k < K; ++k)
    if (levels[k] < 0 || levels[k] >= T) { snprintf(msg, msg_len, "levels[%d] = %d must lie in [0, T = %d)", k, (int)levels[k], T); return -1; }
  return 0;
}

// levels (checked) -> coefficients; abar holds the T entries dhw_schedule gives.  fp32 throughout.
inline std::vector<ScoreLevel> score_level_table(const float* abar, const int32_t* levels, int K) {
  std::vector<ScoreLevel> t((size_t)K);
  for (int k = 0; k < K; ++k) {
    const float a = abar[levels[k]];
    t[(size_t)k] = ScoreLevel{sqrtf(a), sqrtf(1.0f - a), a, SCORE_ITER0 + (int)levels[k]};
  }
  return t;
}
