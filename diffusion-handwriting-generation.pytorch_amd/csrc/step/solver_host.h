// solver_host.h — the host arithmetic of the second-order multistep entries (include/dhw.h: dhw_dpm_coefs, dhw_dpm_update,
// dhw_dpm_sample, dhw_guided_dpm_sample) that needs neither a handle nor a device: the check of `order` and the
// per-step coefficient table, built over ddim_host.h's.  Plain C++ (tests/cpp/solver_host_check.cpp compiles it alone).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ddim/ddim_host.h"

constexpr int DPM_ROW = 9;   // floats per row of dhw_dpm_coefs: kind, c0..c3, k0, k1, c4, c5

// kind of a step: 1 = the DDIM update U along e (+ hist <- x0), 2 = the second-order multistep update
enum DpmKind { DPM_FIRST = 1, DPM_SECOND = 2 };

// Step j of the table: (c0, c1, c2, c3) = (A_j, B_j, A_{j+1}, B_{j+1}) in every row (c2 is also the next forward's sigma);
// (k0, k1, c4, c5) are the second-order step's and 0 in a first-order row.
struct DpmCoef {
  int kind;
  float c0, c1, c2, c3;
  float k0, k1, c4, c5;
};

inline int solver_check_order(int order, char* msg, size_t msg_len) {
  if (order != 1 && order != 2) { snprintf(msg, msg_len, "order = %d must be 1 (DDIM) or 2 (second-order multistep)", order); return -1; }
  return 0;
}

// levels (checked) and order (checked) -> S rows.  Steps 0 and S - 1, and every step of order 1, are first order.  A second-order
// step j (0 < j < S - 1, order 2), in double from the fp32 A, B of ddim_coef_table, each result rounded once to fp32:
//   lambda_j = log(A_j / B_j), h = lambda_{j+1} - lambda_j, r = (lambda_j - lambda_{j-1}) / h,
//   k1 = 1 / (2 r), k0 = 1 + k1, c4 = B_{j+1} / B_j, c5 = -A_{j+1} expm1(-h).
// 0 on success; -1 with the step named in msg when an h or an r is not finite and positive (levels whose fp32 abar coincide, or
// reach 1): such a table is refused.
inline int dpm_coef_table(const float* abar, const int32_t* levels, int S, int order, std::vector<DpmCoef>& out, char* msg, size_t msg_len) {
  const std::vector<DdimCoef> t = ddim_coef_table(abar, levels, S);
  out.assign((size_t)S, DpmCoef{});
  auto lambda = [&](int j) { return log((double)t[(size_t)j].A / (double)t[(size_t)j].B); };
  for (int j = 0; j < S; ++j) {
    DpmCoef& c = out[(size_t)j];
    c.kind = DPM_FIRST;
    c.c0 = t[(size_t)j].A;
    c.c1 = t[(size_t)j].B;
    c.c2 = t[(size_t)j + 1].A;
    c.c3 = t[(size_t)j + 1].B;
    if (order != 2 || j == 0 || j == S - 1) continue;
    const double l0 = lambda(j - 1), l1 = lambda(j), l2 = lambda(j + 1);
    const double h = l2 - l1, r = (l1 - l0) / h;
    if (!(h > 0.0 && std::isfinite(h))) { snprintf(msg, msg_len, "step %d: h = %g (the log-SNR gap to level %d) must be finite and positive", j, h, j + 1); return -1; }
    if (!(r > 0.0 && std::isfinite(r))) { snprintf(msg, msg_len, "step %d: r = %g (the ratio of the log-SNR gaps around level %d) must be finite and positive", j, r, j); return -1; }
    const double k1 = 1.0 / (2.0 * r);
    c.kind = DPM_SECOND;
    c.k0 = (float)(1.0 + k1);
    c.k1 = (float)k1;
    c.c4 = (float)((double)t[(size_t)j + 1].B / (double)t[(size_t)j].B);
    c.c5 = (float)(-(double)t[(size_t)j + 1].A * expm1(-h));
  }
  return 0;
}

// a table row as dhw_dpm_coefs writes it and dhw_dpm_update reads it
inline void dpm_row_pack(const DpmCoef& c, float* row) {
  const float v[DPM_ROW] = {(float)c.kind, c.c0, c.c1, c.c2, c.c3, c.k0, c.k1, c.c4, c.c5};
  for (int i = 0; i < DPM_ROW; ++i) row[i] = v[i];
}

// 0 and the row in c, or -1: kind is neither 1 nor 2
inline int dpm_row_unpack(const float* row, DpmCoef& c, char* msg, size_t msg_len) {
  if (row[0] != 1.0f && row[0] != 2.0f) { snprintf(msg, msg_len, "coef[0] = %g: the kind must be 1 (first order) or 2 (second order)", (double)row[0]); return -1; }
  c = DpmCoef{(int)row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7], row[8]};
  return 0;
}
