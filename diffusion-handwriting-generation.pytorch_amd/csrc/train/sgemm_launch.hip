// sgemm_launch.hip — host side of the training GEMM: tile / split-K / load-form choice (plan_sgemm) and the launchers of one, two
// and up to six GEMMs, over the kernel tables of sgemm_f32 / sgemm_bf16 / sgemm_group .hip.
#include <algorithm>
#include <array>
#include <cstdlib>

#include "sgemm_core.h"

using namespace dhw_train;

// tile / split / load-form choice of one GEMM (shared by the single and the paired launch)
struct SgPlan { int ksplit, kslice; bool am, bk, av, bv, cv, gm32; dim3 grid; };
static hipError_t plan_sgemm(const OpGemm& g, SgPlan& pl) {
  if (g.M < 1 || g.N < 1 || g.K < 1 || g.nzo < 1 || g.nzi < 1 || g.taps < 1) return hipErrorInvalidValue;
  if (g.taps > 1 && (g.K % g.taps || (g.K / g.taps) % GK)) return hipErrorInvalidValue;
  const int tiles_m = (g.M + GT - 1) / GT, tiles_n = (g.N + GT - 1) / GT;
  const long wgs = (long)tiles_m * tiles_n * g.nzo * g.nzi;
  // split K across workgroups while the tile count leaves most of the 256 CUs idle (accumulating outputs only: atomics)
  int ksplit = 1;
  static const long sk_target = getenv("DHW_SGEMM_SPLIT_WGS") ? atol(getenv("DHW_SGEMM_SPLIT_WGS")) : 512;   // (two workgroups per CU: 7.6 vs 7.8 ms per update against 256)
  static const long sk_steps = getenv("DHW_SGEMM_SPLIT_STEPS") ? atol(getenv("DHW_SGEMM_SPLIT_STEPS")) : 8;
  if ((g.act_out || g.film_out) && g.accumulate) return hipErrorInvalidValue;
  if (g.dsilu_of && (g.bias || g.addend)) return hipErrorInvalidValue;   // (a factor on the product alone)
  if (g.accumulate && !g.addend && !g.dsilu_of && wgs < sk_target && g.K >= 2 * sk_steps * GK) ksplit = (int)std::min<long>((sk_target + wgs - 1) / wgs, g.K / (sk_steps * GK));
  if (ksplit < 1) ksplit = 1;
  const int kslice = ((g.K + ksplit - 1) / ksplit + GK - 1) / GK * GK;
  ksplit = (g.K + kslice - 1) / kslice;
  if (tiles_m > 32767 || (long)g.nzo * g.nzi * ksplit > 65535) return hipErrorInvalidValue;
  // lanes run along the index whose stride is the smaller one; 16-byte loads where that stride is 1 and everything is aligned
  const bool am = std::llabs(g.sam) < std::llabs(g.sak), bk = std::llabs(g.sbk) < std::llabs(g.sbn);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  bool av = am ? (g.sam == 1 && g.sak % 4 == 0 && g.M % 4 == 0 && g.a_shift == 0 && g.a_tap_shift == 0)
               : (g.sak == 1 && g.sam % 4 == 0 && g.K % 4 == 0);
  av = av && al16(g.A) && g.sazo % 4 == 0 && g.sazi % 4 == 0;
  bool bv = bk ? (g.sbk == 1 && g.sbn % 4 == 0 && g.K % 4 == 0 && g.b_shift == 0 && g.b_z_shift == 0)
               : (g.sbn == 1 && g.sbk % 4 == 0 && g.N % 4 == 0);
  bv = bv && al16(g.B) && g.sbzo % 4 == 0 && g.sbzi % 4 == 0 && g.sbt % 4 == 0;
  static const bool novec = [] { const char* e = getenv("DHW_SGEMM_SCALAR"); return e && *e == '1'; }();
  if (novec) av = bv = false;
  const bool cv = g.lr > 0 || g.taps > 1 || g.a_shift || g.a_tap_shift || g.b_shift || g.b_z_shift;
  // 32-row tiles where the 64-row tiling would leave CUs idle (fp32, 16-byte-load forms, no split-K): DHW_SGEMM_GM32=0 to compare
  static const bool gm32_on = !(getenv("DHW_SGEMM_GM32") && atoi(getenv("DHW_SGEMM_GM32")) == 0);
  const bool gm32 = gm32_on && av && bv && !g.bf16 && ksplit == 1 && wgs < 224 && g.M > 32;
  pl = SgPlan{ksplit, kslice, am, bk, av, bv, cv, gm32, dim3((unsigned)tiles_n, (unsigned)(gm32 ? (g.M + 31) / 32 : tiles_m), (unsigned)(g.nzo * g.nzi * ksplit))};
  return hipSuccess;
}
static hipError_t launch_planned(const OpGemm& g, const SgPlan& pl, hipStream_t st) {
  static const std::array<SgFn, 64> variants = [] {   // blocks of 16: fp32, bf16, fp32 Conv1d form, bf16 Conv1d form
    const SgFn* f = sgemm_f32_table().variants;
    const SgFn* h = sgemm_bf16_table().variants;
    std::array<SgFn, 64> v;
    for (int i = 0; i < 16; ++i) { v[i] = f[i]; v[16 + i] = h[i]; v[32 + i] = f[16 + i]; v[48 + i] = h[16 + i]; }
    return v;
  }();
  const dim3 block(256);
  if (pl.gm32) {
    static const SgFn* const v32 = sgemm_f32_table().v32;
    hipLaunchKernelGGL(v32[pl.am * 4 + pl.bk * 2 + (pl.cv ? 1 : 0)], pl.grid, block, 0, st, g, pl.ksplit, pl.kslice);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(variants[(pl.cv ? 32 : 0) + (g.bf16 ? 16 : 0) + pl.am * 8 + pl.bk * 4 + pl.av * 2 + pl.bv], pl.grid, block, 0, st, g, pl.ksplit, pl.kslice);
  return hipGetLastError();
}
hipError_t launch_sgemm(const OpGemm& g, hipStream_t st) {
  SgPlan pl;
  const hipError_t e = plan_sgemm(g, pl);
  return e != hipSuccess ? e : launch_planned(g, pl, st);
}
hipError_t launch_sgemm_group(const OpGemm* g, int n, hipStream_t st, int* launches);
// a: a weight gradient (A^T B: m along the lanes of A, n along the lanes of B, 64-row tiles), b: a data gradient (A B with B [K][N]);
// both fp32 with 16-byte loads.  Anything else, or DHW_SGEMM_PAIR=0: two launches.
hipError_t launch_sgemm_pair(const OpGemm& a, const OpGemm& b, hipStream_t st, int* launches) {
  if (launches) *launches = 2;
  SgPlan pa, pb;
  hipError_t e;
  if ((e = plan_sgemm(a, pa)) != hipSuccess || (e = plan_sgemm(b, pb)) != hipSuccess) return e;
  static const bool off = [] { const char* v = getenv("DHW_SGEMM_PAIR"); return v && atoi(v) == 0; }();
  if (!off && a.bf16 && b.bf16) {   // (the mixed-precision mode: through the general grouped kernel)
    const OpGemm two[2] = {a, b};
    return launch_sgemm_group(two, 2, st, launches);
  }
  const bool ok = !off && !a.bf16 && !b.bf16 && !a.stamps && !b.stamps && pa.av && pa.bv && pb.av && pb.bv && pa.am && !pa.bk && !pa.gm32 && !pb.am && !pb.bk;
  if (!ok) {
    if ((e = launch_planned(a, pa, st)) != hipSuccess) return e;
    return launch_planned(b, pb, st);
  }
  static const SgPairFn* const pairs = sgemm_f32_table().pairs;
  const SgGrid ra{pa.grid.x, pa.grid.y, pa.grid.z}, rb{pb.grid.x, pb.grid.y, pb.grid.z};
  const unsigned long n = (unsigned long)ra.gx * ra.gy * ra.gz + (unsigned long)rb.gx * rb.gy * rb.gz;
  if (n > 0x7fffffffUL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pairs[(pa.cv ? 4 : 0) + (pb.cv ? 2 : 0) + (pb.gm32 ? 1 : 0)], dim3((unsigned)n), dim3(256), 0, st, a, pa.ksplit, pa.kslice, ra, b, pb.ksplit, pb.kslice, rb);
  if (launches) *launches = 1;
  return hipGetLastError();
}
// n <= SG_MAXG independent GEMMs: one launch when every one of them is an fp32 16-byte-load form (and not A^T B^T), else one by one.
// DHW_SGEMM_GROUP=0: one by one.
hipError_t launch_sgemm_group(const OpGemm* g, int n, hipStream_t st, int* launches) {
  if (n < 1 || n > SG_MAXG) return hipErrorInvalidValue;
  if (launches) *launches = n;
  SgPlan pl[SG_MAXG];
  hipError_t e;
  static const bool off = [] { const char* v = getenv("DHW_SGEMM_GROUP"); return v && atoi(v) == 0; }();
  bool ok = !off && n > 1;
  for (int i = 0; i < n; ++i) {
    if ((e = plan_sgemm(g[i], pl[i])) != hipSuccess) return e;
    ok = ok && g[i].bf16 == g[0].bf16 && !g[i].stamps && pl[i].av && pl[i].bv && !(pl[i].am && pl[i].bk) && !(g[i].bf16 && pl[i].gm32);
  }
  if (!ok) {
    for (int i = 0; i < n; ++i)
      if ((e = launch_planned(g[i], pl[i], st)) != hipSuccess) return e;
    return hipSuccess;
  }
  SgGroupArgs a{};
  unsigned long tot = 0;
  for (int i = 0; i < SG_MAXG; ++i) {
    if (i < n) {
      a.g[i] = g[i];
      a.ksplit[i] = pl[i].ksplit; a.kslice[i] = pl[i].kslice;
      a.r[i] = SgGrid{pl[i].grid.x, pl[i].grid.y, pl[i].grid.z};
      a.var[i] = ((pl[i].am ? 2 : pl[i].bk ? 1 : 0) * 2 + (pl[i].cv ? 1 : 0)) * 2 + (pl[i].gm32 ? 1 : 0);
      tot += (unsigned long)pl[i].grid.x * pl[i].grid.y * pl[i].grid.z;
    } else {
      a.r[i] = SgGrid{1, 1, 1};
      a.var[i] = -1;
    }
    a.end[i] = (unsigned)tot;
  }
  if (tot > 0x7fffffffUL) return hipErrorInvalidValue;
  static const SgGroupFn* const group = sgemm_group_table().group;   // [0] fp32, [1] bf16 staging
  if (g[0].bf16) hipLaunchKernelGGL(group[1], dim3((unsigned)tot), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(group[0], dim3((unsigned)tot), dim3(256), 0, st, a);
  if (launches) *launches = 1;
  return hipGetLastError();
}
