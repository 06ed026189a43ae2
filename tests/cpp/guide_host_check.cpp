// guide_host_check — stand-alone CPU program behind tests/test_guide_cpu.py: runs the host arithmetic of the guided entries
// that needs no device (csrc/guide/guide_host.h: the checks of the scales, the capacity, the row count and the update kind, and
// the coefficients of the ancestral step).
//   guide_host_check <beta.f32> <abar.f32> <T> <mode> <kind> <B> <L> <max_B> [scale ...]
// prints "err <message>" when a check refuses the arguments, else one "st <c0> <c1> <c2> <c3> <add_noise> <sigma> <sigma_next>"
// line per schedule index i = T-1 .. 0 (floats as hex literals).  A scale is parsed with strtof ("nan", "inf" are accepted
// spellings).  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/guide/guide_host.h"

static bool read_floats(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(float), v.size(), f);
  fclose(f);
  return got == v.size();
}

// a check run twice, once into a buffer shorter than any message: snprintf must truncate, not overrun
template <typename F>
static int twice(F check, char* full, size_t full_len) {
  char msg[8];
  const int rc_short = check(msg, sizeof msg);
  const int rc = check(full, full_len);
  if (rc != rc_short || (rc && (strlen(msg) != sizeof msg - 1 || strncmp(msg, full, sizeof msg - 1)))) exit(3);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  const int T = atoi(argv[3]), mode = atoi(argv[4]), kind = atoi(argv[5]), B = atoi(argv[6]), L = atoi(argv[7]), max_B = atoi(argv[8]);
  std::vector<float> scale;   // exactly the scales given: a check that reads past B of them is an ASan report
  for (int a = 9; a < argc; ++a) scale.push_back(strtof(argv[a], nullptr));
  char full[160];
  if (twice([&](char* m, size_t n) { return guide_check_kind(kind, m, n); }, full, sizeof full)) { printf("err %s\n", full); return 0; }
  if (twice([&](char* m, size_t n) { return guide_check_scale(scale.empty() ? nullptr : scale.data(), (int)scale.size(), m, n); }, full, sizeof full)) {
    printf("err %s\n", full);
    return 0;
  }
  if (twice([&](char* m, size_t n) { return guide_check_capacity(B, max_B, m, n); }, full, sizeof full)) { printf("err %s\n", full); return 0; }
  if (twice([&](char* m, size_t n) { return guide_check_rows(B, L, m, n); }, full, sizeof full)) { printf("err %s\n", full); return 0; }
  if (T < 1 || T > (1 << 20) || (mode != 0 && mode != 1)) return 2;
  std::vector<float> beta((size_t)T), abar((size_t)T);   // exactly T entries: an index out of range is an ASan report
  if (!read_floats(argv[1], beta) || !read_floats(argv[2], abar)) { fprintf(stderr, "cannot read the schedule\n"); return 2; }
  for (int i = T - 1; i >= 0; --i) {
    const GuideStep s = guide_step(mode, beta.data(), abar.data(), i);
    printf("st %a %a %a %a %d %a %a\n", s.c0, s.c1, s.c2, s.c3, s.add_noise, s.sigma, s.sigma_next);
  }
  return 0;
}
