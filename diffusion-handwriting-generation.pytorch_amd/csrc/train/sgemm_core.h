// sgemm_core.h — the training step's strided exact-f32 / bf16 GEMM: tile constants, the workgroup body and the three kernel
// templates built on it (one GEMM, two, up to six per launch).  The instantiations are compiled in three units — sgemm_f32.hip
// (sgemm_tiled_kernel with fp32 staging and the pair kernels), sgemm_bf16.hip (sgemm_tiled_kernel with bf16 staging) and
// sgemm_group.hip (the group kernels) — each of which hands its kernels to the planner (sgemm_launch.hip) as one table of
// function pointers.
//
// Generic fp32 building blocks of the training step (dhw_train.h "dhw_op_*"): everything the denoiser's forward and
// backward need beyond the fused inference kernels, each a plain device-pointer operation so the host side
// (train_model.py) can chain them the way autograd chains the reference's modules.  Correctness first: the GEMM reads its
// operands straight from global memory with caller-given strides (one description covers Linear / Conv1d forward,
// data gradient, weight gradient and the per-head attention products), on the exact-f32 MFMA.
#pragma once
#include <type_traits>

#include "../dhw_common.h"
#include "../dhw_kernels.h"
#include "train_common.h"

namespace dhw_train {

// C[z][m][n] (+)= alpha * sum_k A(z, m, k) * B(z, k, n) (+ bias[n]);  z = zo * nzi + zi (two batch levels, e.g. sample x head)
// with K = taps * Kt and k = tap * Kt + kk (dhw_gemm_desc in include/dhw_train.h):
//   A(z,m,k) = A[zo*sazo + zi*sazi + (m + sa)*sam + kk*sak],  sa = a_shift + tap*a_tap_shift, zero unless (m mod lr) + sa in [0, lr)
//   B(z,k,n) = B[zo*sbzo + zi*sbzi + tap*sbt + (kk + sb)*sbk + n*sbn],  sb = b_shift + zi*b_z_shift, zero unless (kk mod lr) + sb in [0, lr)
// LDS-tiled: one workgroup (4 waves as 2 x 2) = one 64 x 64 tile of C over one K slice; each wave
// owns 32 x 32 (2 x 2 MFMA tiles).  Per 32-wide K step the 64 x 32 A tile and the 32 x 64 B tile go global -> registers
// (issued one step ahead, so their latency hides behind the 32 MFMAs of the current step) -> LDS as As[m][k] / Bs[n][k]
// (row stride 36 floats: the lanes' 16-byte fragment reads fall on disjoint banks) -> two ds_read_b128 per fragment.
// AM / BK pick which index runs along the lanes of a load so that the unit (or smaller) stride is the coalesced one.
// ksplit > 1 (only with accumulate): the K range is cut into slices across workgroups and C is updated with fp32 atomics
// — weight gradients contract over all B*L stroke rows into a few small tiles, and would otherwise run on a few CUs.
constexpr int GT = 64, GK = 32, GS = 36;

// TS = float: exact-f32 MFMA (the default: gradients match the reference's autograd to 1e-5).  TS = bf16_t: the operand tiles
// are rounded to bf16 on their way into LDS and contracted with v_mfma_f32_16x16x32_bf16 (fp32 accumulation, fp32 operands
// in memory, fp32 master weights) — mixed-precision training, 8x fewer MFMA instructions and half the LDS traffic per step.
template <typename TS> constexpr int tile_row = sizeof(TS) == 4 ? GS : 48;   // elements; bf16: 96-byte rows ((stride / 16) mod 4 = 2, gemm_core.h)
DHW_DEV void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
DHW_DEV void st4(bf16_t* p, f32x4 v) {
  bf16_t h[4] = {from_f<bf16_t>(v[0]), from_f<bf16_t>(v[1]), from_f<bf16_t>(v[2]), from_f<bf16_t>(v[3])};
  *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(h);
}
DHW_DEV Frag<float> ld_frag(const float* p) { Frag<float> f; f.lo = *reinterpret_cast<const f32x4*>(p); f.hi = *reinterpret_cast<const f32x4*>(p + 4); return f; }
DHW_DEV Frag<bf16_t> ld_frag(const bf16_t* p) { return frag_load(p); }
// the same 8 k-values out of a k-major fp32 tile: p = &tile[first k][row], rows `stride` floats apart
template <typename TS> DHW_DEV Frag<TS> ld_frag_k(const float* p, int stride);
template <> DHW_DEV Frag<float> ld_frag_k<float>(const float* p, int stride) {
  Frag<float> f;
  f.lo = (f32x4){p[0], p[stride], p[2 * stride], p[3 * stride]};
  f.hi = (f32x4){p[4 * stride], p[5 * stride], p[6 * stride], p[7 * stride]};
  return f;
}
template <> DHW_DEV Frag<bf16_t> ld_frag_k<bf16_t>(const float*, int) { return Frag<bf16_t>{}; }   // (never selected: AKM / BKM are fp32-only)

DHW_DEV float frag_sum(const Frag<float>& f) { return ((f.lo[0] + f.lo[1]) + (f.lo[2] + f.lo[3])) + ((f.hi[0] + f.hi[1]) + (f.hi[2] + f.hi[3])); }
DHW_DEV float frag_sum(const Frag<bf16_t>& f) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += (float)f.v[e];
  return s;
}

// CV: the Conv1d features of the description are in use (taps, row shifts, lr).  The plain variant (every nn.Linear and the
// attention products) compiles without their integer divisions and per-element range tests — the prologue of the general
// form was ~1400 instructions with 19 divisions, as long as the whole K loop of a K = 128 GEMM.
#ifdef DHW_STAMPS
#define SG_STAMP(slot) do { if (g.stamps && bx == 0 && by == gy / 2 && bz == 0 && threadIdx.x == 0) g.stamps[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SG_STAMP(slot) do { } while (0)
#endif
// GM: rows of the output tile, 64 or 32 (columns: always 64).  32-row tiles are for GEMMs whose 64-row tiling would leave CUs
// idle (1 600 - 1 920 rows x 384 columns = 150 - 180 workgroups at the attention level): twice the workgroups, half the K-loop
// work each.
// The body is a device function of the workgroup's tile coordinates (bx = column tile, by = row tile, bz = batch x K slice; gy =
// row tiles, for the diagnostics) and of its LDS block, so that one launch can run two independent GEMMs (sgemm_pair_kernel).
constexpr int SG_BUF = 2 * GT * GS;   // floats per operand buffer (sized for TS = float); a workgroup has two
template <bool AM, bool BK, bool AV, bool BV, typename TS, bool CV, int GM = GT, typename GD = OpGemm>
DHW_DEV void sgemm_body(const GD& g, int ksplit, int kslice, int bx, int by, int bz, int gy, float* smem) {
  static_assert(GM == 64 || GM == 32, "row tile");
  constexpr int MA = GM / 32;   // 16-row MFMA tiles per wave along M
  SG_STAMP(0);
  constexpr int TR = tile_row<TS>;
  // two buffers of operand tiles (TS) — step s is contracted out of one while step s + 1 is staged into the other — then the
  // fp32 output tile
  // fp32 tiles of an operand whose lanes run along m / n (A^T: AM, B [K][N]: !BK) stay k-major in LDS, [k][m] with a row of 66
  // floats: the 16-byte loads go in as two 8-byte stores, conflict-free, and a fragment is eight 4-byte reads (k = 8 q + e: the
  // four lane groups sit 8 rows = 16 banks apart) — instead of transposing with sixteen 4-way-conflicted ds_write_b32 per thread
  // and step (the weight-gradient GEMMs' K step took 1.04 us against 0.74 us for the forms that need no transpose).
  constexpr bool AKM = AM && sizeof(TS) == 4, BKM = !BK && sizeof(TS) == 4;
  constexpr int TRK = 66;
  static_assert(GK * TRK <= GT * GS, "a k-major tile fits the operand's half of a buffer");
  constexpr int BUF = SG_BUF;
  TS* As = reinterpret_cast<TS*>(smem);
  TS* Bs = As + GT * TR;
  constexpr int BUFE = BUF * (int)(sizeof(float) / sizeof(TS));          // the same in elements of TS
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = lane & 15, q = lane >> 4;
  // grid: x = column tile, y = row tile, z = batch index * ksplit + K slice (each division only where its divisor is not 1)
  const int n0 = bx * GT, m0 = by * GM;
  int ks = 0, z = bz, zo = z, zi = 0;
  if (ksplit > 1) { ks = z % ksplit; z /= ksplit; zo = z; }
  if (g.nzi > 1) { zo = z / g.nzi; zi = z - zo * g.nzi; }
  const float* A = g.A + zo * g.sazo + zi * g.sazi;
  const float* B = g.B + zo * g.sbzo + zi * g.sbzi;
  float* C = g.C + zo * g.sczo + zi * g.sczi;
  const int k_begin = ks * kslice, k_end = min(g.K, k_begin + kslice);

  // Staging coordinates of this thread's 8 + 8 elements per K step.  Scalar form (one dword per load):
  //   A: AM (m along lanes): m = t & 63, k = (t >> 6) + 4 j;   else (k along lanes): k = t & 31, m = (t >> 5) + 8 j
  //   B: BK (k along lanes): k = t & 31, n = (t >> 5) + 8 j;   else (n along lanes): n = t & 63, k = (t >> 6) + 4 j
  // Vector form (AV / BV: the lane index has stride exactly 1 and everything is 16-byte aligned), two 16-byte loads:
  //   A: AM: m = 4 (t & 15) .. +3 at k = (t >> 4) + 16 jj;     else: k = 4 (t & 7) .. +3 of row m = (t >> 3) + 32 jj
  //   B: BK: k = 4 (t & 7) .. +3 of column n = (t >> 3) + 32 jj;   else: n = 4 (t & 15) .. +3 at k = (t >> 4) + 16 jj
  // PD K steps of operands are kept in flight in registers (kstep below).
  // Address arithmetic is kept out of the K loop (it was as long as the MFMA work): each element's offset inside its operand
  // is a per-thread 32-bit constant, everything that changes from step to step (k position, tap, row shift) is uniform and
  // goes into the scalar base pointer; the per-step vector work is the validity compares.
  constexpr int PD = 4;
  constexpr int NA = (AV ? 2 : 8) * GM / GT, NB = BV ? 2 : 8;      // loads per thread and step (A: half of them for a 32-row tile)
  float rar[PD][8], rbr[PD][8];
  const int Kt = CV ? g.K / g.taps : g.K;       // taps > 1: Kt is a multiple of GK, so a K step lies inside one tap
  const int b_sh = CV ? g.b_shift + zi * g.b_z_shift : 0;
  const unsigned lr_a = CV && g.lr > 0 ? (unsigned)g.lr : 0x7fffffffu;     // no row shift: every row "in range"
  const unsigned lr_b = CV && b_sh != 0 ? (unsigned)g.lr : 0x7fffffffu;
  // local (tile) coordinates of load j: (am, ak) / (bn, bk); for a vector load the first of its 4 elements
  // (GM = 32 with m along the lanes: 32 m per k row, so 8 / 32 lanes per row and 32 / 8 k rows per pass)
  auto a_m = [&](int j) { return AV ? (AM ? 4 * (t & (GM / 4 - 1)) : (t >> 3) + 32 * j) : (AM ? (t & (GM - 1)) : (t >> 5) + 8 * j); };
  auto a_k = [&](int j) { return AV ? (AM ? (GM == 64 ? (t >> 4) + 16 * j : (t >> 3)) : 4 * (t & 7)) : (AM ? (GM == 64 ? (t >> 6) + 4 * j : (t >> 5) + 8 * j) : (t & 31)); };
  auto b_n = [&](int j) { return BV ? (BK ? (t >> 3) + 32 * j : 4 * (t & 15)) : (BK ? (t >> 5) + 8 * j : (t & 63)); };
  auto b_k = [&](int j) { return BV ? (BK ? 4 * (t & 7) : (t >> 4) + 16 * j) : (BK ? (t & 31) : (t >> 6) + 4 * j); };
  unsigned voa[NA], vob[NB];
  int mla[NA], klb[NB];
  bool mva[NA], nvb[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int m = m0 + a_m(j);
    mva[j] = m < g.M;                            // (a vector load's 4 rows / 4 k are valid together: M, K multiples of 4)
    mla[j] = CV && g.lr > 0 ? m % g.lr : 0;
    voa[j] = (unsigned)(m * (int)g.sam + a_k(j) * (int)g.sak);
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = n0 + b_n(j);
    nvb[j] = n < g.N;
    vob[j] = (unsigned)(b_k(j) * (int)g.sbk + n * (int)g.sbn);
    klb[j] = CV && b_sh != 0 ? (k_begin + b_k(j)) % g.lr : 0;   // row of the contraction index inside its sample (weight gradients)
  }
  int k_next = k_begin;                          // load() is called for consecutive K steps
  // Every load is issued unconditionally at a clamped (always valid) address and its validity bit is kept with the ring slot;
  // stage() zeroes the invalid elements.  Written as `ok ? *p : 0` each load became a branch with s_waitcnt vmcnt(0) behind
  // it, i.e. every K step waited for the loads it had just issued for three steps ahead: the prefetch ring hid nothing and a
  // step cost one full L2 round trip (17-30 us per GEMM of 0.5 GFLOP; r3 ISA).
  unsigned okm[PD];                              // bits 0..7: the A loads of the slot, bits 8..15: the B loads
  // FAST (interior tile of a plain GEMM whose K slice is whole steps — uniform per workgroup): nothing per element at all, the
  // step's base pointers are scalar (past the end of the slice: the first step again — valid memory, never contracted).  The
  // per-element selects, compares and 64-bit address adds of the general form are ~100 VALU instructions per step, and VALU
  // issue stalls the same SIMD's MFMA pipe: a step took 0.85-0.95 us against 0.43 us of MFMA work (tools/bench_sgemm stamps).
  // MODE 2 / 3: the same for a Conv1d GEMM whose tile (2: forward / data gradient, row-shifted A) or K slice (3: weight gradient,
  // row-shifted B) stays inside the operand: unmasked loads at the shifted addresses, one range test per load for the rows that
  // cross a sample edge (zeroed at staging), nothing for the other operand.
  auto load = [&](float (&ra)[8], float (&rb)[8], unsigned& okbits, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    constexpr bool FAST = MODE != 0;
    if constexpr (FAST) {
      const bool past = k_next >= k_end;      // (uniform) a request past the end of the slice: never contracted
      const int k0 = past ? k_begin : k_next;
      k_next += GK;
      const int tap = MODE >= 2 && g.taps > 1 ? k0 / Kt : 0, kb = k0 - tap * Kt;
      const int a_sh = MODE >= 2 ? g.a_shift + tap * g.a_tap_shift : 0;
      const float* Ab = A + (long)a_sh * g.sam + (long)kb * g.sak;
      const float* Bb = B + (MODE >= 2 ? tap * g.sbt : 0) + (long)(kb + b_sh) * g.sbk;
      // (a row that falls outside the operand is always a row that crosses a sample edge — M and K are whole samples — so the one
      // range test also keeps the load inside the buffer: it is issued at the operand's base instead)
      unsigned bits = 0xffffu;
      bool ea[NA], eb[NB];
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        ea[j] = MODE == 2 && (unsigned)(mla[j] + a_sh) >= lr_a;
        if constexpr (MODE == 2) bits &= ~((ea[j] ? 1u : 0u) << j);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        eb[j] = MODE == 3 && (unsigned)(klb[j] + b_sh) >= lr_b;
        if constexpr (MODE == 3) {
          bits &= ~((eb[j] ? 1u : 0u) << (8 + j));
          klb[j] += GK;
          if (g.lr >= GK) klb[j] -= klb[j] >= g.lr ? g.lr : 0;
          else klb[j] %= g.lr;
        }
      }
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const float* src = MODE == 2 && ea[j] ? A : Ab + voa[j];
        if constexpr (AV) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(src);
          ra[4 * j] = v[0]; ra[4 * j + 1] = v[1]; ra[4 * j + 2] = v[2]; ra[4 * j + 3] = v[3];
        } else {
          ra[j] = *src;
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        // (MODE 3 past the end: klb has moved on while the address went back to the first step — everything from the base)
        const float* src = MODE == 3 && (eb[j] || past) ? B : Bb + vob[j];
        if constexpr (BV) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(src);
          rb[4 * j] = v[0]; rb[4 * j + 1] = v[1]; rb[4 * j + 2] = v[2]; rb[4 * j + 3] = v[3];
        } else {
          rb[j] = *src;
        }
      }
      okbits = bits;
      return;
    }
    const int k0 = k_next;
    k_next += GK;
    const int tap = CV && g.taps > 1 ? k0 / Kt : 0, kb = k0 - tap * Kt;
    const int a_sh = CV ? g.a_shift + tap * g.a_tap_shift : 0;
    const int krem = k_end - k0;                 // <= 0 past the end of the slice: every element invalid
    const float* Ab = A + (long)a_sh * g.sam + (long)kb * g.sak;
    const float* Bb = B + (CV ? tap * g.sbt : 0) + (long)(kb + b_sh) * g.sbk;
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const bool ok = mva[j] && a_k(j) < krem && (!CV || (unsigned)(mla[j] + a_sh) < lr_a);
      bits |= (ok ? 1u : 0u) << j;
      const float* src = ok ? Ab + voa[j] : A;
      if constexpr (AV) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
        ra[4 * j] = v[0]; ra[4 * j + 1] = v[1]; ra[4 * j + 2] = v[2]; ra[4 * j + 3] = v[3];
      } else {
        ra[j] = *src;
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const bool okb = nvb[j] && b_k(j) < krem && (!CV || (unsigned)(klb[j] + b_sh) < lr_b);
      bits |= (okb ? 1u : 0u) << (8 + j);
      const float* src = okb ? Bb + vob[j] : B;
      if constexpr (BV) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
        rb[4 * j] = v[0]; rb[4 * j + 1] = v[1]; rb[4 * j + 2] = v[2]; rb[4 * j + 3] = v[3];
      } else {
        rb[j] = *src;
      }
      if (CV && b_sh != 0) {                     // uniform
        klb[j] += GK;
        if (g.lr >= GK) klb[j] -= klb[j] >= g.lr ? g.lr : 0;   // (uniform; samples shorter than a K step: the general form)
        else klb[j] %= g.lr;
      }
    }
    okbits = bits;
  };
  auto stage = [&](const float (&ra)[8], const float (&rb)[8], unsigned bits, int buf, auto modec) {
    constexpr int MODE = decltype(modec)::value;
    TS* As = reinterpret_cast<TS*>(smem) + buf * BUFE;
    TS* Bs = As + GT * TR;
    auto z = [&](int bit, float v) {   // (bit is a constant after unrolling: A loads 0..7, B loads 8..15)
      if constexpr (MODE == 1) return v;
      else if ((MODE == 2 && bit >= 8) || (MODE == 3 && bit < 8)) return v;
      else return (bits >> bit) & 1u ? v : 0.f;
    };
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if constexpr (AKM) {
        float* Ak = reinterpret_cast<float*>(As);
        if constexpr (AV) {
          float2* d = reinterpret_cast<float2*>(Ak + a_k(j) * TRK + a_m(j));
          d[0] = make_float2(z(j, ra[4 * j]), z(j, ra[4 * j + 1]));
          d[1] = make_float2(z(j, ra[4 * j + 2]), z(j, ra[4 * j + 3]));
        } else Ak[a_k(j) * TRK + a_m(j)] = z(j, ra[j]);
      } else if constexpr (AV && !AM) st4(As + a_m(j) * TR + a_k(j), (f32x4){z(j, ra[4 * j]), z(j, ra[4 * j + 1]), z(j, ra[4 * j + 2]), z(j, ra[4 * j + 3])});
      else if constexpr (AV) {
#pragma unroll
        for (int e = 0; e < 4; ++e) As[(a_m(j) + e) * TR + a_k(j)] = from_f<TS>(z(j, ra[4 * j + e]));
      } else As[a_m(j) * TR + a_k(j)] = from_f<TS>(z(j, ra[j]));
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if constexpr (BKM) {
        float* Bk = reinterpret_cast<float*>(Bs);
        if constexpr (BV) {
          float2* d = reinterpret_cast<float2*>(Bk + b_k(j) * TRK + b_n(j));
          d[0] = make_float2(z(8 + j, rb[4 * j]), z(8 + j, rb[4 * j + 1]));
          d[1] = make_float2(z(8 + j, rb[4 * j + 2]), z(8 + j, rb[4 * j + 3]));
        } else Bk[b_k(j) * TRK + b_n(j)] = z(8 + j, rb[j]);
      } else if constexpr (BV && BK) st4(Bs + b_n(j) * TR + b_k(j), (f32x4){z(8 + j, rb[4 * j]), z(8 + j, rb[4 * j + 1]), z(8 + j, rb[4 * j + 2]), z(8 + j, rb[4 * j + 3])});
      else if constexpr (BV) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(b_n(j) + e) * TR + b_k(j)] = from_f<TS>(z(8 + j, rb[4 * j + e]));
      } else Bs[b_n(j) * TR + b_k(j)] = from_f<TS>(z(8 + j, rb[j]));
    }
  };

  f32x4 acc[MA][2];
#pragma unroll
  for (int a = 0; a < MA; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0, 0, 0, 0};
  const int wm = (wave >> 1) * (GM / 2), wn = (wave & 1) * 32;

  // bias gradient riding on the weight-gradient GEMM (g.rowsum): the waves that hold the A fragments of the first column tile
  // of batch 0 also add them up — 16 additions per lane and step instead of a second pass over dy (colsum_kernel: one launch
  // per Linear / Conv1d, 8.7 % of the update)
  const bool rs_on = g.rowsum != nullptr && n0 == 0 && z == 0 && wn == 0;   // (wave-uniform)
  float rs[MA] = {};
  // Step s (ring slot p = s mod PD, LDS buffer p & 1): request step s + PD, read this step's fragments, and stage step
  // s + 1 into the other buffer between the two halves of the MFMA work — the matrix pipe runs while the wave does the
  // staging's selects and LDS writes; ONE barrier per step (everybody's reads of this buffer and writes of the next are done).
  // (Fragments of step s + 1 read ahead into a second register set, tile s + 2 staged meanwhile: no faster per step and
  // 8.1 vs 7.6 ms per update for the registers it costs.)
  auto run = [&](auto fastc) {
    SG_STAMP(1);
#pragma unroll
    for (int p = 0; p < PD; ++p) load(rar[p], rbr[p], okm[p], fastc);
    SG_STAMP(2);
    stage(rar[0], rbr[0], okm[0], 0, fastc);
    __syncthreads();
    SG_STAMP(3);
    auto kstep = [&](auto pc) {
      constexpr int p = decltype(pc)::value, pn = (p + 1) % PD;
      const TS* Ac = reinterpret_cast<const TS*>(smem) + (p & 1) * BUFE;
      const TS* Bc = Ac + GT * TR;
      load(rar[p], rbr[p], okm[p], fastc);   // slot p was staged one step ago: it takes step s + PD (past k_end: clamped, all-zero)
      Frag<TS> fa[MA], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        if (a < MA) {
          if constexpr (AKM) fa[a % MA] = ld_frag_k<TS>(reinterpret_cast<const float*>(Ac) + 8 * q * TRK + wm + 16 * a + i, TRK);
          else fa[a % MA] = ld_frag(Ac + (wm + 16 * a + i) * TR + 8 * q);
        }
        if constexpr (BKM) fb[a] = ld_frag_k<TS>(reinterpret_cast<const float*>(Bc) + 8 * q * TRK + wn + 16 * a + i, TRK);
        else fb[a] = ld_frag(Bc + (wn + 16 * a + i) * TR + 8 * q);
      }
      mma32(acc[0][0], fa[0], fb[0]);
      if constexpr (MA == 1) stage(rar[pn], rbr[pn], okm[pn], pn & 1, fastc);
      mma32(acc[0][1], fa[0], fb[1]);
      if constexpr (MA == 2) {
        stage(rar[pn], rbr[pn], okm[pn], pn & 1, fastc);
        mma32(acc[1][0], fa[1], fb[0]);
        mma32(acc[1][1], fa[1], fb[1]);
      }
      if (rs_on) {
#pragma unroll
        for (int a = 0; a < MA; ++a) rs[a] += frag_sum(fa[a]);
      }
      __syncthreads();
    };
    // Steady state: PD steps per iteration with NO branch inside — hipcc's s_waitcnt insertion loses track of which loads have
    // landed at every control-flow merge and then waits for (nearly) all of them before it reuses a ring register, which
    // serialises the ring just like the vmcnt(0) above.  The remaining steps (up to PD, the last one partial) follow with their tests.
    int kb = k_begin;
    for (; kb + PD * GK <= k_end; kb += PD * GK) {
      kstep(std::integral_constant<int, 0>{});
      kstep(std::integral_constant<int, 1>{});
      kstep(std::integral_constant<int, 2>{});
      kstep(std::integral_constant<int, 3>{});
    }
    static_assert(PD == 4, "the unrolled ring above");
    if (kb < k_end) kstep(std::integral_constant<int, 0>{});
    if (kb + GK < k_end) kstep(std::integral_constant<int, 1>{});
    if (kb + 2 * GK < k_end) kstep(std::integral_constant<int, 2>{});
    if (kb + 3 * GK < k_end) kstep(std::integral_constant<int, 3>{});   // (fewer than PD * GK elements left can still be PD steps, the last one partial)
  };
  // (uniform over the workgroup)
  const bool interior = m0 + GM <= g.M && n0 + GT <= g.N && (k_end - k_begin) % GK == 0;
  if constexpr (!CV) {
    if (interior) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
  } else {
    int mode = 0;
    const bool ashift = g.a_shift != 0 || g.a_tap_shift != 0, bshift = g.b_shift != 0 || g.b_z_shift != 0;
    if (interior && g.lr > 0) {
      if (ashift && !bshift && g.M % g.lr == 0) mode = 2;
      else if (bshift && !ashift && g.taps == 1 && g.K % g.lr == 0) mode = 3;
    }
    if (mode == 2) run(std::integral_constant<int, 2>{});
    else if (mode == 3) run(std::integral_constant<int, 3>{});
    else run(std::integral_constant<int, 0>{});
  }

  // acc[a][b][r] = C[m0 + wm + 16 a + 4 q + r][n0 + wn + 16 b + i].  The tile goes through LDS so that a wave-instruction
  // writes 64 consecutive columns of one row (256 contiguous bytes when scn = 1) instead of 16 columns of 4 rows: fp32
  // atomics run at their full rate only for whole 256-byte wave-instructions (MI355X_MICROARCH.md, atomics), and the split-K
  // weight gradients are made of them.
  SG_STAMP(4);
  if (rs_on) {   // lanes i, i + 16, i + 32, i + 48 hold the four k-quarters of row wm + 16 a + i
#pragma unroll
    for (int a = 0; a < MA; ++a) {
      float v = rs[a];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      const int m = m0 + wm + 16 * a + i;
      if (q == 0 && m < g.M) atomicAdd(g.rowsum + m, v);
    }
  }
  constexpr int CS = GT + 4;   // (16-byte rows for the vector path below; conflict-free for the accumulator writes either way)
  static_assert(GT * CS <= 2 * BUF, "the output tile reuses the operand tiles");
  // (the last K step ended with a barrier: every fragment read and staging write of the operand buffers is done)
  float* Cs = smem;
#pragma unroll
  for (int a = 0; a < MA; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cs[(wm + 16 * a + 4 * q + r) * CS + wn + 16 * b + i] = acc[a][b][r];
  __syncthreads();
  // interior tile of a row-major output without split-K: 16 bytes per lane, 4 store instructions per thread instead of 16
  const float* Dd = g.addend ? g.addend + zo * g.sczo + zi * g.sczi : nullptr;   // (ksplit == 1 with an addend / act_out: launch_sgemm)
  float* Ao = g.act_out ? g.act_out + zo * g.sczo + zi * g.sczi : nullptr;
  const float* Du = g.dsilu_of ? g.dsilu_of + zo * g.sczo + zi * g.sczi : nullptr;
  // FiLM (+ SiLU) (+ addend) of the written value as a further output (unbatched GEMMs: the ConvBlock's convolutions and fc)
  float* Fo = g.film_out;
  const float* Fa = g.film_add;
  const bool vec_out = ksplit == 1 && g.scn == 1 && (g.scm & 3) == 0 && m0 + GM <= g.M && n0 + GT <= g.N &&
                       ((reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(Dd) | reinterpret_cast<uintptr_t>(Ao) | reinterpret_cast<uintptr_t>(Du) | (g.bias ? reinterpret_cast<uintptr_t>(g.bias) : 0) |
                         reinterpret_cast<uintptr_t>(Fo) | reinterpret_cast<uintptr_t>(Fa) | (Fo ? (reinterpret_cast<uintptr_t>(g.film_g) | reinterpret_cast<uintptr_t>(g.film_b) | (uintptr_t)(g.film_ps * 4)) : 0)) & 15) == 0;   // uniform
  if (vec_out) {
    const int c4 = 4 * (t & 15);
    const f32x4 bias = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + n0 + c4) : (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int it = 0; it < GM / 16; ++it) {
      const int rr = (t >> 4) + 16 * it;
      f32x4* c = reinterpret_cast<f32x4*>(C + (long)(m0 + rr) * g.scm + n0 + c4);
      f32x4 v = *reinterpret_cast<const f32x4*>(Cs + rr * CS + c4) * g.alpha + bias;
      if (Dd) v += *reinterpret_cast<const f32x4*>(Dd + (long)(m0 + rr) * g.scm + n0 + c4);
      if (Du) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(Du + (long)(m0 + rr) * g.scm + n0 + c4);
        v = v * (f32x4){dsilu_f(u[0]), dsilu_f(u[1]), dsilu_f(u[2]), dsilu_f(u[3])};
      }
      *c = g.accumulate ? *c + v : v;
      if (Ao) *reinterpret_cast<f32x4*>(Ao + (long)(m0 + rr) * g.scm + n0 + c4) = (f32x4){silu_f(v[0]), silu_f(v[1]), silu_f(v[2]), silu_f(v[3])};
      if (Fo) {
        const long fb = (long)((m0 + rr) / g.film_rows) * g.film_ps + n0 + c4;
        f32x4 f = v * *reinterpret_cast<const f32x4*>(g.film_g + fb) + *reinterpret_cast<const f32x4*>(g.film_b + fb);
        if (g.film_act) f = (f32x4){silu_f(f[0]), silu_f(f[1]), silu_f(f[2]), silu_f(f[3])};
        if (Fa) f += *reinterpret_cast<const f32x4*>(Fa + (long)(m0 + rr) * g.scm + n0 + c4);
        *reinterpret_cast<f32x4*>(Fo + (long)(m0 + rr) * g.scm + n0 + c4) = f;
      }
    }
  } else {
    const int n = n0 + lane;
    if (n < g.N) {
      const float bias = (g.bias && ks == 0) ? g.bias[n] : 0.f;
      float* cn = C + (long)n * g.scn;
      const int rot = ks * 20;   // K slices of one tile start at different rows: their atomics meet on different cache lines
      for (int r0 = wave; r0 < GM; r0 += 4) {
        const int rr = (r0 + rot) & (GM - 1);
        const int m = m0 + rr;
        if (m >= g.M) continue;
        float* c = cn + (long)m * g.scm;
        float v = g.alpha * Cs[rr * CS + lane] + bias;
        if (Dd) v += Dd[(long)n * g.scn + (long)m * g.scm];
        if (Du) v *= dsilu_f(Du[(long)n * g.scn + (long)m * g.scm]);
        if (ksplit > 1) atomicAdd(c, v);
        else *c = g.accumulate ? *c + v : v;
        if (Ao) Ao[(long)n * g.scn + (long)m * g.scm] = silu_f(v);
        if (Fo) {
          const long fb = (long)(m / g.film_rows) * g.film_ps + n;
          float f = v * g.film_g[fb] + g.film_b[fb];
          if (g.film_act) f = silu_f(f);
          if (Fa) f += Fa[(long)n * g.scn + (long)m * g.scm];
          Fo[(long)n * g.scn + (long)m * g.scm] = f;
        }
      }
    }
  }
  SG_STAMP(5);
}

template <bool AM, bool BK, bool AV, bool BV, typename TS, bool CV, int GM = GT>
__global__ __launch_bounds__(256) void sgemm_tiled_kernel(const OpGemm g, int ksplit, int kslice) {
  __shared__ __attribute__((aligned(16))) float smem[2 * SG_BUF];
  sgemm_body<AM, BK, AV, BV, TS, CV, GM>(g, ksplit, kslice, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, smem);
}

// TWO independent GEMMs in one launch (round 4): workgroups [0, n0) run the first, the rest the second.  A layer's weight-gradient
// and data-gradient GEMMs (both read dy, neither reads the other's output) were two of the update's 306 GEMM launches each, and
// every launch of this graph lives >= 4.5 us whatever it computes (the smallest kernels of the trace); as one launch the
// second GEMM's workgroups also fill the CUs that the first one's split-K tail leaves idle.  VA / VB: SgV<...> below (fp32,
// 16-byte-load forms).  The first GEMM's workgroups are dispatched first: the longer one (the weight gradient) goes there.
template <bool AM, bool BK, bool CV, int GM>
struct SgV {
  static DHW_DEV void run(const OpGemm& g, int ksplit, int kslice, int bx, int by, int bz, int gy, float* smem) {
    sgemm_body<AM, BK, true, true, float, CV, GM>(g, ksplit, kslice, bx, by, bz, gy, smem);
  }
};
struct SgGrid { unsigned gx, gy, gz; };
template <typename VA, typename VB>
__global__ __launch_bounds__(256) void sgemm_pair_kernel(const OpGemm g0, int ks0, int kl0, SgGrid r0, const OpGemm g1, int ks1, int kl1, SgGrid r1) {
  __shared__ __attribute__((aligned(16))) float smem[2 * SG_BUF];
  unsigned id = blockIdx.x;
  const unsigned n0 = r0.gx * r0.gy * r0.gz;
  if (id < n0) {
    const unsigned t = id / r0.gx;
    VA::run(g0, ks0, kl0, (int)(id - t * r0.gx), (int)(t % r0.gy), (int)(t / r0.gy), (int)r0.gy, smem);
  } else {
    id -= n0;
    const unsigned t = id / r1.gx;
    VB::run(g1, ks1, kl1, (int)(id - t * r1.gx), (int)(t % r1.gy), (int)(t / r1.gy), (int)r1.gy, smem);
  }
}

// UP TO SIX independent GEMMs in one launch, any mix of the fp32 16-byte-load forms (the q / k / v projections of an attention
// and, backward, their three weight- and three data-gradient GEMMs; dV with dP, dQ with dK).  The descriptors travel by value in
// the kernel-argument segment and are read from there through a constant-address-space pointer (scalar loads, no private copy of
// the one a workgroup picks); a workgroup finds its GEMM from the cumulative workgroup counts.
constexpr int SG_MAXG = 6;
struct SgGroupArgs {
  OpGemm g[SG_MAXG];
  int ksplit[SG_MAXG], kslice[SG_MAXG];
  SgGrid r[SG_MAXG];
  unsigned end[SG_MAXG];   // cumulative workgroup counts (entries past the last GEMM: the total)
  int var[SG_MAXG];        // form: ((A^T ? 2 : B^T ? 1 : 0) * 2 + conv) * 2 + (32-row tiles)
};
typedef const __attribute__((address_space(4))) SgGroupArgs* SgGroupPtr;
typedef const __attribute__((address_space(4))) OpGemm SgDescC;
template <typename TS>   // float: exact-f32 MFMA; bf16_t: operands rounded to bf16 at staging (every member of a group has the same mode)
__global__ __launch_bounds__(256) void sgemm_group_kernel(const SgGroupArgs by_value) {
  __shared__ __attribute__((aligned(16))) float smem[2 * SG_BUF];
  SgGroupPtr a = (SgGroupPtr)__builtin_amdgcn_kernarg_segment_ptr();   // = &by_value
  unsigned id = blockIdx.x;
  int i = 0;
#pragma unroll
  for (int k = 0; k < SG_MAXG - 1; ++k) i += id >= a->end[k] ? 1 : 0;
  if (i) id -= a->end[i - 1];
  const unsigned gx = a->r[i].gx, gy = a->r[i].gy, t = id / gx;
  const int bx = (int)(id - t * gx), by = (int)(t % gy), bz = (int)(t / gy), ks = a->ksplit[i], kl = a->kslice[i];
  SgDescC& g = a->g[i];
#define DHW_SGG(V_, AM_, BK_, CV_, GM_) case V_: sgemm_body<AM_, BK_, true, true, TS, CV_, GM_, SgDescC>(g, ks, kl, bx, by, bz, (int)gy, smem); break
  switch (a->var[i]) {
    DHW_SGG(0, false, false, false, 64); DHW_SGG(1, false, false, false, 32); DHW_SGG(2, false, false, true, 64); DHW_SGG(3, false, false, true, 32);
    DHW_SGG(4, false, true, false, 64);  DHW_SGG(5, false, true, false, 32);  DHW_SGG(6, false, true, true, 64);  DHW_SGG(7, false, true, true, 32);
    DHW_SGG(8, true, false, false, 64);  DHW_SGG(9, true, false, false, 32);  DHW_SGG(10, true, false, true, 64); DHW_SGG(11, true, false, true, 32);
    default: break;
  }
#undef DHW_SGG
}

// The units' tables, as launch_planned / launch_sgemm_pair / launch_sgemm_group index them.
using SgFn = void (*)(const OpGemm, int, int);
using SgPairFn = void (*)(const OpGemm, int, int, SgGrid, const OpGemm, int, int, SgGrid);
using SgGroupFn = void (*)(const SgGroupArgs);
#define DHW_SG4(AM_, BK_, TS_, CV_) sgemm_tiled_kernel<AM_, BK_, false, false, TS_, CV_>, sgemm_tiled_kernel<AM_, BK_, false, true, TS_, CV_>, \
                                    sgemm_tiled_kernel<AM_, BK_, true, false, TS_, CV_>, sgemm_tiled_kernel<AM_, BK_, true, true, TS_, CV_>
#define DHW_SG16(TS_, CV_) DHW_SG4(false, false, TS_, CV_), DHW_SG4(false, true, TS_, CV_), DHW_SG4(true, false, TS_, CV_), DHW_SG4(true, true, TS_, CV_)
struct SgF32Table {
  SgFn variants[32];     // [cv * 16 + am * 8 + bk * 4 + av * 2 + bv]
  SgFn v32[8];           // 32-row tiles: [am * 4 + bk * 2 + cv]
  SgPairFn pairs[8];     // [cva * 4 + cvb * 2 + (32-row second member)]
};
struct SgBf16Table { SgFn variants[32]; };
struct SgGroupTable { SgGroupFn group[2]; };   // [bf16]
#pragma GCC visibility push(hidden)
const SgF32Table& sgemm_f32_table();       // sgemm_f32.hip
const SgBf16Table& sgemm_bf16_table();     // sgemm_bf16.hip
const SgGroupTable& sgemm_group_table();   // sgemm_group.hip
#pragma GCC visibility pop

}  // namespace dhw_train
