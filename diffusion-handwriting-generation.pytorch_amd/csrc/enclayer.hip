// enclayer.hip — the stroke side of one EncoderLayer (reference model.py:37-58) in TWO launches instead of
// eight.  A workgroup (8 waves) owns 64 / 32 / 16 stroke rows of one sample (enc_plan_bm, plan/tile_plan.h: enough tiles for every CU);
// every intermediate of its rows lives in LDS.  The only hand-off through global memory is the one the algorithm
// forces: self-attention needs the K/V of ALL rows of the sample, so the layer is cut between the q/k/v projection
// and the attention — and since everything between two self-attentions is row-local, enc_bc<NEXT> goes on with the
// next layer's enc_a (enc5: via AvgPool1d + att_dense) on the tile it holds, so a chain of layers costs one launch each.
//
//   enc_a : q1 = Wq(x+PE) -> cross-attention over the text keys -> dense -> LN -> FiLM1 -> +x = x2
//           -> [q2|k2|v2] = W(x2 (+PE))                       (writes x2, qk2, vt2)
//   enc_bc: self-attention(q2,k2,v2) -> dense -> +x2 -> LN -> FiLM2 = x3 -> ffn1 (SiLU) -> ffn2 -> +x3
//           -> LN -> FiLM3 = out (+ AvgPool1d(2) side output)
//
// GEMM stages: every wave covers all rows and 1/WN of the channels (no two waves stream the same weights), weights
// streamed from L2 in fragment order (gemm_core.h).  Attention stages: K/V blocks staged in LDS, wave = 16 rows x
// one or two heads (attn_core.h).  Workgroup ids are XCD-aware (xcd_swizzle.h): a sample's tiles share one L2.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "enc_bc_core.h"
#include "plan/tile_plan.h"

namespace {

template <typename T, int DM, int BM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void enc_a_kernel(const EncLayerParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles = (p.Lk + BM - 1) / BM;
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);   // the row tiles of one sample run on one XCD (shared K/V in its L2)
  enc_a_tile<T, DM, BM>(p, bid / tiles, (bid % tiles) * BM, smem);
}

template <typename T, int DM, int BM, int NEXT = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void enc_bc_kernel(const EncLayerParams p, const EncChain nx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles = (p.Lk + BM - 1) / BM;
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);   // the row tiles of one sample run on one XCD (shared K/V in its L2)
  enc_bc_body<T, DM, BM, NEXT>(p, nx, bid / tiles, (bid % tiles) * BM, smem);
}

template <typename T, int DM, int BM, int NEXT = 0>
hipError_t launch_bc(const EncLayerParams& p, const EncChain& nx, hipStream_t st) {
  const int tiles = (p.Lk + BM - 1) / BM;
  constexpr size_t lds = lds_bc_chain_bytes<T, DM, BM, NEXT>();
  static_assert(lds <= 160 * 1024, "enc_bc tile does not fit LDS");
  hipLaunchKernelGGL((enc_bc_kernel<T, DM, BM, NEXT>), dim3(p.B * tiles), dim3(512), lds, st, p, nx);
  return hipGetLastError();
}

// variants with a compiled chain: mode 1 for the attention layers (DM = 384, tiles up to 32 rows: LDS), mode 2 for enc5
template <typename T, int DM, int BM>
constexpr bool has_chain(int mode) {   // (LDS: the chained layer's text K/V block sits behind the three stage tiles; bf16 only)
  return sizeof(T) == 2 && ((mode == 1 && DM == 384 && BM <= 32) || (mode == 2 && DM == 256 && BM == 32));
}

// does the (element type, width, row tile) combination fit the 160 KiB of LDS in both halves of the layer?
template <typename T, int DM, int BM>
constexpr bool fits() { return lds_a_bytes<T, DM, BM>() <= 160 * 1024 && lds_bc_bytes<T, DM, BM>() <= 160 * 1024 && (DM % 128 == 0 || BM >= 32); }

template <typename T, int DM, int BM>
hipError_t launch_pair(const EncLayerParams& p, int which, hipStream_t st, const EncChain* chain) {
  if constexpr (!fits<T, DM, BM>()) {
    return hipErrorInvalidValue;
  } else {
  const int tiles = (p.Lk + BM - 1) / BM;
  if (which == 0) {
    constexpr size_t lds = lds_a_bytes<T, DM, BM>();
    hipLaunchKernelGGL((enc_a_kernel<T, DM, BM>), dim3(p.B * tiles), dim3(512), lds, st, p);
    return hipGetLastError();
  }
  {
    if (chain && chain->mode) {
      if (chain->a.x) return hipErrorInvalidValue;   // the chained layer reads its x tile from LDS
      if constexpr (has_chain<T, DM, BM>(1)) { if (chain->mode == 1 && chain->a.d == DM) return launch_bc<T, DM, BM, 1>(p, *chain, st); }
      if constexpr (has_chain<T, DM, BM>(2)) { if (chain->mode == 2 && chain->a.d == 384 && !(p.Lk & 1)) return launch_bc<T, DM, BM, 2>(p, *chain, st); }
      return hipErrorInvalidValue;
    }
    return launch_bc<T, DM, BM, 0>(p, EncChain{}, st);
  }
  }
}

template <typename T, int DM, int BM, int NEXT>
hipError_t attr_bc() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(enc_bc_kernel<T, DM, BM, NEXT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

template <typename T, int DM, int BM>
hipError_t attr() {
  if constexpr (fits<T, DM, BM>()) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(enc_a_kernel<T, DM, BM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if ((e = attr_bc<T, DM, BM, 0>()) != hipSuccess) return e;
    if constexpr (has_chain<T, DM, BM>(1)) { if ((e = attr_bc<T, DM, BM, 1>()) != hipSuccess) return e; }
    if constexpr (has_chain<T, DM, BM>(2)) { if ((e = attr_bc<T, DM, BM, 2>()) != hipSuccess) return e; }
  }
  return hipSuccess;
}

template <int F32> using elem_t = std::conditional_t<F32 != 0, float, bf16_t>;

// per row of ENC_VARIANTS (plan/tile_plan.h): fits(), and the chain modes has_chain() gives it (bit 0 = mode 1, bit 1 = mode 2)
#define X(F32, DM, BM) fits<elem_t<F32>, DM, BM>(),
constexpr bool FIT[] = {DHW_ENC_VARIANTS(X)};
#undef X
#define X(F32, DM, BM) has_chain<elem_t<F32>, DM, BM>(1) | has_chain<elem_t<F32>, DM, BM>(2) << 1,
constexpr int CHAIN_MODES[] = {DHW_ENC_VARIANTS(X)};
#undef X

int plan_bm(int prec, int d, int B, int Lk, int bm_min) { return enc_plan_bm(prec != PREC_BF16, d, B, Lk, bm_min, enc_knobs(d), FIT); }

}  // namespace

hipError_t enclayer_init() {
  hipError_t e;
#define X(F32, DM, BM) if ((e = attr<elem_t<F32>, DM, BM>()) != hipSuccess) return e;
  DHW_ENC_VARIANTS(X)
#undef X
  return hipSuccess;
}

bool enclayer_supported(int prec, int d, int heads) {
  const bool f32_fused = !(getenv("DHW_FUSE_F32") && atoi(getenv("DHW_FUSE_F32")) == 0);   // A/B: one launch per GEMM in fp32
  return (prec == PREC_BF16 || (prec == PREC_F32 && f32_fused)) && (d == 192 || d == 256 || d == 384) && heads * 64 == d;
}

// which: 0 = enc_a (cross attention half + q/k/v projection), 1 = enc_bc (self attention + FFN half)
bool enclayer_chain_supported(int prec, int d, int B, int Lk, int mode, int d_next) {
  if (prec != PREC_BF16) return false;
  if (mode == 1) return d == 384 && d_next == 384 && plan_bm(prec, 384, B, Lk, 0) <= 32;
  if (mode == 2) return d == 256 && d_next == 384 && (Lk & 1) == 0 && plan_bm(prec, 256, B, Lk, 32) == 32;   // (with bm_min = 32)
  return false;
}

hipError_t launch_enclayer(int prec, const EncLayerParams& p, int which, hipStream_t st, const EncChain* chain) {
  if (!enclayer_supported(prec, p.d, p.heads) || (p.pool && (p.Lk & 1)) || (chain && chain->mode && which != 1)) return hipErrorInvalidValue;
  if (prec == PREC_F32) {
    if (chain && chain->mode) return hipErrorInvalidValue;
    chain = nullptr;
  }
  switch (enc_find({prec != PREC_BF16, p.d, plan_bm(prec, p.d, p.B, p.Lk, p.bm_min)})) {
#define X(F32, DM, BM) case enc_find({F32, DM, BM}): return launch_pair<elem_t<F32>, DM, BM>(p, which, st, chain);
    DHW_ENC_VARIANTS(X)
#undef X
  }
  return hipErrorInvalidValue;
}

#ifndef DHW_STORE_RT   // (the uniform build alone exports the queries behind dhw_debug_enc_plan / dhw_debug_tile_variants)
int enclayer_plan_bm(int prec, int d, int B, int Lk, int bm_min, const EncKnobs& k) { return enc_plan_bm(prec != PREC_BF16, d, B, Lk, bm_min, k, FIT); }
void enclayer_variant_facts(int i, int* fits, int* chain_modes) { *fits = FIT[i], *chain_modes = CHAIN_MODES[i]; }
#endif
