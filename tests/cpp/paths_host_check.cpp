// paths_host_check — stand-alone CPU program behind tests/test_paths_cpu.py: runs what dhw_paths decides without a device
// (csrc/paths/paths_host.h: the workspace size and every argument rule).
//   paths_host_check <N> <L> <P> <H> <W> <lines_per_page> <margin_left> <margin_top> <pitch> <scale> <smooth> <tol> <rounds>
//                    <null mask> <misalign mask> <workspace bytes short>
// null / misalign mask bits: 1 strokes, 2 points_out, 4 index_out, 8 counts_out, 16 scale_out, 32 boxes_out, 64 workspace,
// 128 lens, 256 slots (a NULL lens or slots is allowed).  Prints "err <message>" when a rule refuses the arguments, else
// "ok <workspace bytes>".  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/paths/paths_host.h"

int main(int argc, char** argv) {
  if (argc != 17) return 2;
  const int N = atoi(argv[1]), L = atoi(argv[2]);
  const PageGeometry g{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), strtof(argv[7], nullptr), strtof(argv[8], nullptr),
                       strtof(argv[9], nullptr), 0.f, strtof(argv[10], nullptr)};   // (a line width of 0: dhw_paths has none, the rules must not look)
  const PathsOptions o{atoi(argv[11]), strtof(argv[12], nullptr), atoi(argv[13])};
  const int nullmask = atoi(argv[14]), mis = atoi(argv[15]);
  const long long shortby = atoll(argv[16]);
  alignas(16) static char buf[9][64];   // nine distinct 16-byte aligned addresses: the rules compare pointers, they never read
  const void* ptr[9];
  for (int k = 0; k < 9; ++k) ptr[k] = (nullmask >> k) & 1 ? nullptr : buf[k] + (((mis >> k) & 1) ? 2 : 0);
  const size_t need = paths_workspace_bytes(N, L);
  const size_t have = shortby > 0 && (size_t)shortby <= need ? need - (size_t)shortby : need;
  char msg[8];   // (shorter than any message: snprintf must truncate, not overrun)
  char full[256];
  const int rc_short = paths_check_args(ptr[0], ptr[7], ptr[8], N, L, g, o, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], have, msg, sizeof msg);
  const int rc = paths_check_args(ptr[0], ptr[7], ptr[8], N, L, g, o, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], have, full, sizeof full);
  if (rc != rc_short || (rc && (strlen(msg) != sizeof msg - 1 || strncmp(msg, full, sizeof msg - 1)))) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  if (need != (((size_t)N * 4 + 15) & ~(size_t)15)) return 3;
  printf("ok %zu\n", need);
  return 0;
}
