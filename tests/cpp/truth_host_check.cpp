// truth_host_check — stand-alone CPU program behind tests/test_truth_cpu.py: runs what dhw_truth decides without a device
// (csrc/truth/truth_host.h: the workspace size and every argument rule).
//   truth_host_check <N> <L> <G> <P> <H> <W> <lines_per_page> <margin_left> <margin_top> <pitch> <line_width> <scale>
//                    <null mask> <misalign mask> <workspace bytes short>
// null / misalign mask bits: 1 strokes, 2 groups, 4 boxes_out, 8 spans_out, 16 scale_out, 32 workspace, 64 labels_out,
// 128 lens, 256 slots (a NULL labels_out, lens or slots is allowed).  Prints "err <message>" when a rule refuses the
// arguments, else "ok <workspace bytes>".  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/truth/truth_host.h"

int main(int argc, char** argv) {
  if (argc != 16) return 2;
  const int N = atoi(argv[1]), L = atoi(argv[2]), G = atoi(argv[3]);
  const PageGeometry g{atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), strtof(argv[8], nullptr), strtof(argv[9], nullptr),
                       strtof(argv[10], nullptr), strtof(argv[11], nullptr), strtof(argv[12], nullptr)};
  const int nullmask = atoi(argv[13]), mis = atoi(argv[14]);
  const long long shortby = atoll(argv[15]);
  alignas(16) static char buf[9][64];   // nine distinct 16-byte aligned addresses: the rules compare pointers, they never read
  const void* ptr[9];
  for (int k = 0; k < 9; ++k) ptr[k] = (nullmask >> k) & 1 ? nullptr : buf[k] + (((mis >> k) & 1) ? 2 : 0);
  const size_t need = truth_workspace_bytes(N, L, G);
  const size_t have = shortby > 0 && (size_t)shortby <= need ? need - (size_t)shortby : need;
  char msg[8];   // (shorter than any message: snprintf must truncate, not overrun)
  char full[256];
  const int rc_short = truth_check_args(ptr[0], ptr[7], ptr[8], ptr[1], N, L, G, g, ptr[2], ptr[3], ptr[6], ptr[4], ptr[5], have, msg, sizeof msg);
  const int rc = truth_check_args(ptr[0], ptr[7], ptr[8], ptr[1], N, L, G, g, ptr[2], ptr[3], ptr[6], ptr[4], ptr[5], have, full, sizeof full);
  if (rc != rc_short || (rc && (strlen(msg) != sizeof msg - 1 || strncmp(msg, full, sizeof msg - 1)))) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  if (need != (((size_t)N * 32 + (size_t)N * L * 20 + 15) & ~(size_t)15)) return 3;
  printf("ok %zu\n", need);
  return 0;
}
