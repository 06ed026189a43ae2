// solver_host_check — stand-alone CPU program behind tests/test_solver_cpu.py: runs the host arithmetic of the second-order
// multistep entries that needs no device (csrc/step/solver_host.h: the check of order and the coefficient table, over ddim_host.h's
// level checks).
//   solver_host_check <abar.f32> <T> <order> [level ...]
// prints "err <message>" when a check refuses the arguments, else one "co <kind> <c0> <c1> <c2> <c3> <k0> <k1> <c4> <c5>" line per
// step (S of them, floats as hex literals), each row having gone through dpm_row_pack / dpm_row_unpack.  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/step/solver_host.h"

// the same refusal into a buffer shorter than any message: snprintf must truncate, not overrun
static bool same_prefix(int rc, int rc_short, const char* msg, size_t msg_size, const char* full) {
  return rc == rc_short && (!rc || (strlen(msg) == msg_size - 1 && !strncmp(msg, full, msg_size - 1)));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int T = atoi(argv[2]), order = atoi(argv[3]);
  std::vector<int32_t> levels;
  for (int a = 4; a < argc; ++a) levels.push_back((int32_t)atoi(argv[a]));
  std::vector<float> abar(T > 0 && T <= (1 << 20) ? (size_t)T : 0);   // exactly T entries: a level the checks let through out of range is an ASan report
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const size_t got = fread(abar.data(), sizeof(float), abar.size(), f);
  fclose(f);
  if (got != abar.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  char msg[8];
  char full[160];
  const int32_t* lv = levels.empty() ? nullptr : levels.data();
  const int S = (int)levels.size();
  int rc = ddim_check_levels(T, lv, S, full, sizeof full);
  if (rc) { printf("err %s\n", full); return 0; }
  rc = solver_check_order(order, full, sizeof full);
  if (!same_prefix(rc, solver_check_order(order, msg, sizeof msg), msg, sizeof msg, full)) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  std::vector<DpmCoef> t, t_short;
  rc = dpm_coef_table(abar.data(), lv, S, order, t, full, sizeof full);
  if (!same_prefix(rc, dpm_coef_table(abar.data(), lv, S, order, t_short, msg, sizeof msg), msg, sizeof msg, full)) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  if ((int)t.size() != S) return 3;
  for (const DpmCoef& c : t) {
    float row[DPM_ROW];
    DpmCoef back{};
    dpm_row_pack(c, row);
    if (dpm_row_unpack(row, back, full, sizeof full) || memcmp(&back, &c, sizeof c)) return 3;
    printf("co %d %a %a %a %a %a %a %a %a\n", c.kind, c.c0, c.c1, c.c2, c.c3, c.k0, c.k1, c.c4, c.c5);
  }
  float bad[DPM_ROW] = {3.0f};
  DpmCoef none{};
  rc = dpm_row_unpack(bad, none, full, sizeof full);
  if (rc != -1 || !same_prefix(rc, dpm_row_unpack(bad, none, msg, sizeof msg), msg, sizeof msg, full) || !strstr(full, "coef[0] = 3")) return 3;
  return 0;
}
