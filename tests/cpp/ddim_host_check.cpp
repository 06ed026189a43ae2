// ddim_host_check — stand-alone CPU program behind tests/test_ddim_cpu.py: runs the host arithmetic of dhw_ddim_sample /
// dhw_ddim_invert that needs no device (csrc/ddim/ddim_host.h: the checks of T, S, levels and iters, and the coefficient table).
//   ddim_host_check <abar.f32> <T> <iters> [level ...]
// prints "err <message>" when a check refuses the arguments, else one "co <A> <B>" line per table entry (S + 1 of them, floats
// as hex literals).  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/ddim/ddim_host.h"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int T = atoi(argv[2]), iters = atoi(argv[3]);
  std::vector<int32_t> levels;
  for (int a = 4; a < argc; ++a) levels.push_back((int32_t)atoi(argv[a]));
  std::vector<float> abar(T > 0 && T <= (1 << 20) ? (size_t)T : 0);   // exactly T entries: a level the checks let through out of range is an ASan report
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const size_t got = fread(abar.data(), sizeof(float), abar.size(), f);
  fclose(f);
  if (got != abar.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  char msg[8];   // (shorter than any message: snprintf must truncate, not overrun)
  char full[160];
  const int32_t* lv = levels.empty() ? nullptr : levels.data();
  const int S = (int)levels.size();
  const int rc_short = ddim_check_levels(T, lv, S, msg, sizeof msg);
  int rc = ddim_check_levels(T, lv, S, full, sizeof full);
  if (rc != rc_short || (rc && (strlen(msg) != sizeof msg - 1 || strncmp(msg, full, sizeof msg - 1)))) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  const int ri_short = ddim_check_iters(iters, msg, sizeof msg);
  rc = ddim_check_iters(iters, full, sizeof full);
  if (rc != ri_short || (rc && (strlen(msg) != sizeof msg - 1 || strncmp(msg, full, sizeof msg - 1)))) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  const std::vector<DdimCoef> t = ddim_coef_table(abar.data(), lv, S);
  if ((int)t.size() != S + 1) return 3;
  for (const DdimCoef& c : t) printf("co %a %a\n", c.A, c.B);
  return 0;
}
