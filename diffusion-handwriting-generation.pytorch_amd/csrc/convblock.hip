// convblock.hip — one whole ConvBlock (reference cnn.py:64-87) as a single kernel:
//
//     out = FiLM3(fc(SiLU(FiLM2(conv2(SiLU(FiLM1(conv1(SiLU(x))))))))) + conv_skip(x)
//
// A workgroup owns BM-2 consecutive stroke rows of one sample.  x (raw and SiLU'd, +2 halo rows each side) is
// staged into LDS once — for enc1 it is computed on the fly from the (dx,dy) strokes (input Linear(2->C),
// model.py:139), so the sampler state never round-trips through an activation buffer; conv1 -> h1 and
// conv2 -> h2 never leave LDS; the k=3 taps of every conv read row-shifted views of the staged tiles; fc and
// conv_skip accumulate into the same MFMA accumulators with the FiLM3 affine applied in between.  Weights
// stream from L2 in MFMA-fragment order through a register ring that is re-filled for the NEXT stage before
// the current stage's epilogue (gemm_core.h).  The output tile goes through LDS so global stores are whole
// coalesced rows (+ the AvgPool1d side output).  Replaces three launches and the HBM/L2 round trips of h1/h2.
//
// bf16: 8 waves (2 per SIMD), 62-row tiles (126 at full resolution, 46 or 32 at the L/4 level: conv_plan, plan/tile_plan.h).  fp32 (parity
// mode): 4 waves, 30-row tiles (LDS budget).  Decoder blocks (UPC) evaluate Upsample(low) + skip_conv(h) (model.py:169-175)
// as one more 3-tap GEMM stage in front; dec1 evaluates the eps / pen heads and the scheduler step from its fp32 tile;
// CH = 1 continues into the next EncoderLayer's first half on the output tile (enc_a_core.h; off by default).
#include <algorithm>
#include <type_traits>
#include "convblock_core.h"
#include "plan/tile_plan.h"

namespace {

template <typename T, int BM, int CO, int NW, int OCC = 1, int UPC = 0, int CH = 0, int CIN = 0, int TIGHT = 0, int PP = 0>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(OCC * NW / 4, (OCC * NW / 4) < 2 ? 2 : OCC * NW / 4)))
void convblock_kernel(const ConvBlockParams p, const EncChain nx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BMO = TIGHT == 2 ? BM : BM - 2 - 2 * TIGHT;
  const int tiles = (p.L + BMO - 1) / BMO;
  // XCD-aware workgroup id, the same sample -> XCD assignment in every fused kernel of the model: a sample's activations
  // are then handed from kernel to kernel inside one XCD's L2 (measured: a 98 KB tile written by the previous kernel on
  // the same XCD is read in 1.6 us, from another XCD in 3.8 us — tools/bench_handoff.cpp)
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  convblock_body<T, BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP>(p, nx, bid / tiles, (bid % tiles) * BMO, smem);
}

template <typename T, int BM, int CO, int NW, int OCC = 1, int UPC = 0, int CH = 0, int CIN = 0, int TIGHT = 0, int PP = 0>
hipError_t launch_t(const ConvBlockParams& p, hipStream_t st, const EncChain* nx = nullptr) {
  size_t lds = lds_bytes<T, BM, CO>(p.Cin, UPC ? p.up_cin : 0, TIGHT == 2 ? BM + 16 : BM);
  if (CH) lds = std::max(lds, (size_t)2 * BM * tile_stride<T>(CO) + 2 * 8 * BM * sizeof(float) + enc_a_text_kv_bytes<T, CO, BM>() + enc_a_param_bytes<T, CO>());
  if (lds > 160 * 1024 || (UPC && (p.Cin != UPC || p.up_cin % 32)) || (CH != 0) != (nx != nullptr)) return hipErrorInvalidValue;
  if (CIN && (p.Cin != CIN || (UPC && p.up_cin != up_skip_width<UPC>()))) return hipErrorInvalidValue;
  constexpr int BMO = TIGHT == 2 ? BM : BM - 2 - 2 * TIGHT;
  const int tiles = (p.L + BMO - 1) / BMO;
  hipLaunchKernelGGL((convblock_kernel<T, BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP>), dim3(p.B * tiles), dim3(NW * 64), lds, st, p, nx ? *nx : EncChain{});
  return hipGetLastError();
}

template <int F32> using elem_t = std::conditional_t<F32 != 0, float, bf16_t>;

// CONV_VARIANTS[idx] (plan/tile_plan.h) -> its launch_t
hipError_t launch_variant(int idx, const ConvBlockParams& p, hipStream_t st, const EncChain* nx) {
  switch (idx) {
#define X(F32, ...) case conv_find({F32, __VA_ARGS__}): return launch_t<elem_t<F32>, __VA_ARGS__>(p, st, nx);
    DHW_CONV_VARIANTS(X)
#undef X
  }
  return hipErrorInvalidValue;
}

// what the tile plan looks at; the LDS facts come from lds_bytes<>() here
ConvShape shape_of(int prec, int B, int L, int Cin, int Cout, bool up, int up_cin, bool chain) {
  ConvShape s{prec != PREC_BF16, B, L, Cin, Cout, up, up_cin, chain, false, false};
  s.tall_fits = lds_bytes<bf16_t, 128, 128>(Cin, up ? up_cin : 0) <= 160 * 1024;
  s.occ2_fits = Cout == 128 ? lds_bytes<bf16_t, 64, 128>(Cin) <= 80 * 1024 : Cout == 192 && lds_bytes<bf16_t, 64, 192>(Cin) <= 80 * 1024;
  return s;
}
ConvShape shape_of(int prec, const ConvBlockParams& p, bool chain) { return shape_of(prec, p.B, p.L, p.Cin, p.Cout, p.up_h != nullptr, p.up_cin, chain); }

}  // namespace

hipError_t convblock_init() {
  hipError_t e;
#define X(F32, ...)                                                                                                       \
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(convblock_kernel<elem_t<F32>, __VA_ARGS__>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
  if (e != hipSuccess) return e;
  DHW_CONV_VARIANTS(X)
#undef X
  return hipSuccess;
}

hipError_t launch_convblock(int prec, const ConvBlockParams& p_in, hipStream_t st) {
  ConvBlockParams p = p_in;
  p.stagger = conv_stagger(p.stagger);
  if (p.Cin % 32 || (p.L & 1) || (p.pool && p.out_f32) || (p.fuse_heads && !p.out_f32) || (!p.out && !p.fuse_heads)) return hipErrorInvalidValue;
  // a decoder block with the fused Upsample + skip_conv input stage (bf16 only: the plan refuses it in fp32)
  if (p.up_h && (p.strokes || !p.up_w || !p.up_b || !p.up_low)) return hipErrorInvalidValue;
  return launch_variant(conv_plan(shape_of(prec, p, false), conv_knobs()), p, st, nullptr);
}

// The encoder-side blocks in front of an EncoderLayer (enc2 -> enc3, enc4 -> enc5): bf16, no fused input stage, no fp32
// output, the block's width is the layer's width; and the plan has a chain variant for the shape (none under a forced tile).
bool convblock_chain_supported(int prec, const ConvBlockParams& p, const EncChain& chain) {
  if (prec != PREC_BF16 || chain.mode != 1 || chain.a.x || p.up_h || p.strokes || p.out_f32 || p.fuse_heads) return false;
  if (chain.a.d != p.Cout || chain.a.Lk != p.L || chain.a.B != p.B || (p.L & 1)) return false;
  return conv_plan(shape_of(prec, p, true), conv_knobs()) >= 0 && enclayer_supported(prec, chain.a.d, chain.a.heads);
}

// Whether continuing this block into the next EncoderLayer's first half is a measured WIN for its launch geometry (the default of
// DHW_CHAIN_CONV for enc4 -> enc5.a): only on the asymmetric 32-row tiles, which are the layer's own tiling (r5: 18.02 -> 17.89 ms
// same-box, profiles/r05_enc4_chain_ab.log; on the 46-row tiles the chain measured slower in rounds 1 and 3).
bool convblock_chain_auto(const ConvBlockParams& p) {
  const int i = conv_plan(shape_of(PREC_BF16, p, true), conv_knobs());   // (the chain's plan for this shape is the asymmetric variant)
  return i >= 0 && CONV_VARIANTS[i].TIGHT == 2;
}

hipError_t launch_convblock_chain(int prec, const ConvBlockParams& p, const EncChain& chain, hipStream_t st) {
  if (!convblock_chain_supported(prec, p, chain) || p.Cin % 32 || (!p.out)) return hipErrorInvalidValue;
  return launch_variant(conv_plan(shape_of(prec, p, true), conv_knobs()), p, st, &chain);
}

#ifndef DHW_STORE_RT   // (the uniform build alone exports the query behind dhw_debug_conv_plan)
int convblock_plan(int prec, int B, int L, int Cin, int Cout, int up_cin, bool chain, const ConvKnobs& k) {   // up_cin = 0: no fused input stage
  return conv_plan(shape_of(prec, B, L, Cin, Cout, up_cin != 0, up_cin, chain), k);
}
#endif
