// page_host_check — stand-alone CPU program behind tests/test_page_cpu.py: runs what dhw_page decides without a device
// (csrc/page/page_host.h: the workspace size and every argument rule).
//   page_host_check <N> <L> <P> <H> <W> <lines_per_page> <margin_left> <margin_top> <pitch> <line_width> <scale>
//                   <null mask> <misalign mask> <workspace bytes short>
// null / misalign mask bits: 1 strokes, 2 pages, 4 scale_out, 8 boxes_out, 16 workspace.  Prints "err <message>" when a rule
// refuses the arguments, else "ok <workspace bytes>".  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/page/page_host.h"

int main(int argc, char** argv) {
  if (argc != 15) return 2;
  const int N = atoi(argv[1]), L = atoi(argv[2]);
  const PageGeometry g{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), strtof(argv[7], nullptr), strtof(argv[8], nullptr),
                       strtof(argv[9], nullptr), strtof(argv[10], nullptr), strtof(argv[11], nullptr)};
  const int nullmask = atoi(argv[12]), mis = atoi(argv[13]);
  const long long shortby = atoll(argv[14]);
  alignas(16) static char buf[5][64];   // five distinct 16-byte aligned addresses: the rules compare pointers, they never read
  const void* ptr[5];
  for (int k = 0; k < 5; ++k) ptr[k] = (nullmask >> k) & 1 ? nullptr : buf[k] + (((mis >> k) & 1) ? 2 : 0);
  const size_t need = page_workspace_bytes(N, L);
  const size_t have = shortby > 0 && (size_t)shortby <= need ? need - (size_t)shortby : need;
  char msg[8];   // (shorter than any message: snprintf must truncate, not overrun)
  char full[256];
  const int rc_short = page_check_args(ptr[0], N, L, g, ptr[1], ptr[2], ptr[3], ptr[4], have, msg, sizeof msg);
  const int rc = page_check_args(ptr[0], N, L, g, ptr[1], ptr[2], ptr[3], ptr[4], have, full, sizeof full);
  if (rc != rc_short || (rc && (strlen(msg) != sizeof msg - 1 || strncmp(msg, full, sizeof msg - 1)))) return 3;
  if (rc) { printf("err %s\n", full); return 0; }
  if (need != (size_t)N * PAGE_HEADER_BYTES + (size_t)N * (size_t)L * PAGE_SEGMENT_BYTES) return 3;
  printf("ok %zu\n", need);
  return 0;
}
