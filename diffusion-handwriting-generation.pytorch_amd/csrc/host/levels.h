// host/levels.h — the check of (T, levels) that dhw_score and the ddim entries (include/dhw.h) share.  Plain C++: needs
// neither a handle nor a device (tests/cpp/score_host_check.cpp and ddim_host_check.cpp compile it through score_host.h / ddim_host.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

constexpr int MAX_T = 1 << 29;   // the largest schedule an entry accepts

// 0 on success, else -1 with the offending argument named in msg.  n levels are expected; count_name is what the entry calls
// n ("K", "S").  strictly_decreasing: each level must lie below the one before it (the ddim entries; dhw_score takes any order).
inline int check_levels(int T, const int32_t* levels, int n, const char* count_name, bool strictly_decreasing, char* msg, size_t msg_len) {
  if (T < 1 || T > MAX_T) { snprintf(msg, msg_len, "T = %d must lie in [1, 2^29]", T); return -1; }
  if (n < 1 || n > T) { snprintf(msg, msg_len, "%s = %d must lie in [1, T = %d]", count_name, n, T); return -1; }
  if (!levels) { snprintf(msg, msg_len, "levels is NULL (%s = %d entries expected)", count_name, n); return -1; }
  for (int j = 0; j < n; ++j) {
    if (levels[j] < 0 || levels[j] >= T) { snprintf(msg, msg_len, "levels[%d] = %d must lie in [0, T = %d)", j, (int)levels[j], T); return -1; }
    if (strictly_decreasing && j > 0 && levels[j] >= levels[j - 1]) {
      snprintf(msg, msg_len, "levels[%d] = %d is not below levels[%d] = %d: levels must be strictly decreasing", j, (int)levels[j], j - 1, (int)levels[j - 1]);
      return -1;
    }
  }
  return 0;
}
