// guide_host.h — the host arithmetic of the guided entries (include/dhw.h: dhw_guided_ddim_sample, dhw_guided_sample,
// dhw_guide_update) that needs neither a handle nor a device: the checks of the scales, of the doubled batch against the
// handle's capacity and of the update kind, and the per-iteration coefficients of the ancestral step.  Plain C++
// (tests/cpp/guide_host_check.cpp compiles it alone).  The level checks and the DDIM coefficient table are ddim_host.h's.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../ddim/ddim_host.h"

constexpr float GUIDE_MAX_SCALE = 64.0f;   // scales lie in [0, 64]

// which update follows the combine (dhw_guide_update's `kind`)
enum GuideKind { GUIDE_DDIM = 0, GUIDE_NEW = 1, GUIDE_STANDARD = 2 };

inline int guide_check_kind(int kind, char* msg, size_t msg_len) {
  if (kind < GUIDE_DDIM || kind > GUIDE_STANDARD) { snprintf(msg, msg_len, "kind = %d must be 0 (ddim), 1 (new) or 2 (standard)", kind); return -1; }
  return 0;
}

// every scale finite and in [0, GUIDE_MAX_SCALE]  (written so that a NaN fails the range test)
inline int guide_check_scale(const float* scale, int B, char* msg, size_t msg_len) {
  if (!scale) { snprintf(msg, msg_len, "null pointer (scale)"); return -1; }
  for (int b = 0; b < B; ++b)
    if (!(scale[b] >= 0.0f && scale[b] <= GUIDE_MAX_SCALE)) {
      snprintf(msg, msg_len, "scale[%d] = %g must be finite and lie in [0, %g]", b, (double)scale[b], (double)GUIDE_MAX_SCALE);
      return -1;
    }
  return 0;
}

// a guided call of B samples is one forward over 2B rows
inline int guide_check_capacity(int B, int max_B, char* msg, size_t msg_len) {
  if (B < 1 || B > max_B / 2) {
    snprintf(msg, msg_len, "B = %d: a guided call runs 2B = %lld rows through the denoiser, the handle holds max_B = %d", B, 2LL * B, max_B);
    return -1;
  }
  return 0;
}

// 2 B L rows are indexed with 32 bits
inline int guide_check_rows(int B, int L, char* msg, size_t msg_len) {
  if (B < 1 || L < 1 || 2LL * B * L > 0x7fffffffLL) { snprintf(msg, msg_len, "shape out of range: B=%d L=%d (both >= 1, 2 * B * L below 2^31)", B, L); return -1; }
  return 0;
}

// The ancestral step of schedule index i (0 <= i < T), as dhw_sample computes it on the host in fp32 (sampler/sample.cpp):
//   mode 0 ("new"):      x = (x - c0 e) / c1 + z c2                  c0 = sqrtf(1 - abar_i), c1 = sqrtf(1 - beta_i), c2 = sqrtf(1 - abar_next)
//   mode 1 ("standard"): x = c1 (x - (c3 e) / c0) [+ c2 z, i != 0]   c1 = 1 / sqrtf(1 - beta_i), c2 = sqrtf(beta_i), c3 = beta_i
// abar_next = abar[i - 1] for i > 1 and 1 otherwise (inference.py:87); sigma_next = sqrtf(abar[i - 1]), the level of the next forward.
struct GuideStep {
  float c0, c1, c2, c3;
  int add_noise;
  float sigma, sigma_next;
};

inline GuideStep guide_step(int mode, const float* beta, const float* abar, int i) {
  GuideStep s{};
  const float a = abar[i], b = beta[i];
  const float a_next = i > 1 ? abar[i - 1] : 1.0f;
  s.c0 = sqrtf(1.0f - a);
  if (mode == 0) {
    s.c1 = sqrtf(1.0f - b);
    s.c2 = sqrtf(1.0f - a_next);
    s.add_noise = 1;
  } else {
    s.c1 = 1.0f / sqrtf(1.0f - b);
    s.c2 = sqrtf(b);
    s.c3 = b;
    s.add_noise = i != 0;
  }
  s.sigma = sqrtf(a);
  s.sigma_next = i > 0 ? sqrtf(abar[i - 1]) : 0.0f;
  return s;
}
