// plan/tile_plan.h — which compiled ConvBlock / EncoderLayer kernel variant a launch runs: the variant lists and the rule, as pure
// host logic (no HIP, no environment: dhw_debug_conv_plan / dhw_debug_enc_plan run it without a device, tests/cpp/tile_plan_check.cpp
// on its own).  convblock.hip / enclayer.hip and their ragged/ and policy/ builds generate their init lists and their dispatch from
// the lists here and ask the rule here, with the knobs plan/tile_knobs.cpp reads from the environment.
#pragma once

// ---------------------------------------------------------------- the compiled variants: the ONLY place one is named
// convblock_kernel<T, BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP> (csrc/convblock.hip), T = float where F32 else bf16_t
#define DHW_CONV_VARIANTS(X)                                                                                                        \
  /* run-time input width (decoder blocks without the fused input stage, experiments) */                                            \
  X(0, 64, 128, 8, 1, 0, 0, 0, 0, 0) X(0, 128, 128, 8, 1, 0, 0, 0, 0, 0) X(0, 64, 128, 8, 2, 0, 0, 128, 0, 0)                       \
  X(0, 64, 192, 8, 2, 0, 0, 128, 0, 0) X(0, 64, 192, 8, 1, 0, 0, 0, 0, 0)                                                           \
  X(0, 64, 256, 8, 1, 0, 0, 0, 0, 0) X(0, 32, 256, 8, 1, 0, 0, 0, 0, 0) X(0, 48, 256, 8, 1, 0, 0, 0, 0, 0)                          \
  /* encoder blocks, input width compiled in */                                                                                     \
  X(0, 64, 128, 8, 1, 0, 0, 128, 0, 0) X(0, 128, 128, 8, 1, 0, 0, 128, 0, 0) X(0, 64, 192, 8, 1, 0, 0, 128, 0, 0)                   \
  X(0, 64, 256, 8, 1, 0, 0, 192, 0, 0) X(0, 48, 256, 8, 1, 0, 0, 192, 0, 0)                                                         \
  /* decoder blocks with the fused Upsample + skip_conv input stage */                                                              \
  X(0, 64, 128, 8, 1, 192, 0, 192, 0, 0) X(0, 128, 128, 8, 1, 192, 0, 192, 0, 0) X(0, 64, 192, 8, 1, 256, 0, 256, 0, 0)             \
  X(0, 64, 256, 8, 1, 384, 0, 384, 0, 0) X(0, 48, 256, 8, 1, 384, 0, 384, 0, 0)                                                     \
  /* ... writing BM - 4 rows per tile (convblock_core.h, TIGHT) */                                                                  \
  X(0, 128, 128, 8, 1, 192, 0, 192, 1, 0) X(0, 48, 256, 8, 1, 384, 0, 384, 1, 0)                                                    \
  /* the tall tiles with the row halves one phase apart (PP) */                                                                     \
  X(0, 128, 128, 8, 1, 0, 0, 128, 0, 1) X(0, 128, 128, 8, 1, 192, 0, 192, 1, 1) X(0, 128, 128, 8, 1, 192, 0, 192, 0, 1)             \
  /* 32-row tiles of the widest blocks, conv1 over 48 rows (TIGHT = 2) */                                                           \
  X(0, 32, 256, 8, 1, 0, 0, 192, 2, 0) X(0, 32, 256, 8, 1, 384, 0, 384, 2, 0)                                                       \
  /* encoder blocks that continue into the next EncoderLayer's first half */                                                        \
  X(0, 64, 192, 8, 1, 0, 1, 128, 0, 0) X(0, 48, 256, 8, 1, 0, 1, 192, 0, 0) X(0, 64, 256, 8, 1, 0, 1, 192, 0, 0)                    \
  /* ... on the asymmetric 32-row tiles (the layer's own 32-row tiling: enc4 -> enc5.a) */                                          \
  X(0, 32, 256, 8, 1, 0, 1, 192, 2, 0)                                                                                              \
  /* fp32 parity mode */                                                                                                            \
  X(1, 32, 128, 4, 1, 0, 0, 0, 0, 0) X(1, 32, 192, 4, 1, 0, 0, 0, 0, 0) X(1, 32, 256, 4, 1, 0, 0, 0, 0, 0)

// enc_a_kernel<T, DM, BM> / enc_bc_kernel<T, DM, BM, NEXT> (csrc/enclayer.hip: fits() says which rows exist, has_chain() which NEXT)
#define DHW_ENC_VARIANTS(X)                                                                                      \
  X(0, 192, 64) X(0, 256, 64) X(0, 384, 64) X(0, 192, 32) X(0, 256, 32) X(0, 384, 32) X(0, 256, 16) X(0, 384, 16) \
  /* fp32 parity mode: the same kernels (exact-f32 MFMA), the row tiles that fit LDS */                          \
  X(1, 192, 64) X(1, 192, 32) X(1, 256, 32) X(1, 256, 16) X(1, 384, 16)

struct ConvVariant {
  int f32, BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP;
  constexpr int rows() const { return TIGHT == 2 ? BM : BM - 2 - 2 * TIGHT; }   // output rows per tile (BMO, convblock_core.h)
  void row(int out[11]) const {   // the template arguments, then rows(): what include/dhw_debug.h reports
    const int r[11] = {f32, BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP, rows()};
    for (int i = 0; i < 11; ++i) out[i] = r[i];
  }
  constexpr bool operator==(const ConvVariant& o) const {
    return f32 == o.f32 && BM == o.BM && CO == o.CO && NW == o.NW && OCC == o.OCC && UPC == o.UPC && CH == o.CH && CIN == o.CIN && TIGHT == o.TIGHT && PP == o.PP;
  }
};
struct EncVariant {
  int f32, DM, BM;
  constexpr bool operator==(const EncVariant& o) const { return f32 == o.f32 && DM == o.DM && BM == o.BM; }
};
#define DHW_ROW(...) {__VA_ARGS__},
constexpr ConvVariant CONV_VARIANTS[] = {DHW_CONV_VARIANTS(DHW_ROW)};
constexpr EncVariant ENC_VARIANTS[] = {DHW_ENC_VARIANTS(DHW_ROW)};
#undef DHW_ROW
constexpr int N_CONV_VARIANTS = sizeof(CONV_VARIANTS) / sizeof(CONV_VARIANTS[0]);
constexpr int N_ENC_VARIANTS = sizeof(ENC_VARIANTS) / sizeof(ENC_VARIANTS[0]);

// row of the table that holds v, or -1: a launch of a variant nobody compiled is refused, never attempted
constexpr int conv_find(const ConvVariant& v) {
  for (int i = 0; i < N_CONV_VARIANTS; ++i)
    if (CONV_VARIANTS[i] == v) return i;
  return -1;
}
constexpr int enc_find(const EncVariant& v) {
  for (int i = 0; i < N_ENC_VARIANTS; ++i)
    if (ENC_VARIANTS[i] == v) return i;
  return -1;
}

// ---------------------------------------------------------------- ConvBlock
// What the rule may look at.  No per-sample lengths: the uniform, ragged and store-policy launches of one shape run one tiling.
struct ConvShape {
  bool f32;
  int B, L, Cin, Cout;
  bool up;          // decoder block with the fused Upsample + skip_conv input stage ...
  int up_cin;       // ... and the width of its skip-connection activation
  bool chain;       // continues into the next EncoderLayer's first half (launch_convblock_chain)
  // LDS facts, computed by the caller from lds_bytes<>() (convblock_core.h):
  bool tall_fits;   // lds_bytes<bf16_t, 128, 128>(Cin[, up_cin]) <= 160 KiB
  bool occ2_fits;   // lds_bytes<bf16_t, 64, Cout>(Cin) <= 80 KiB: two workgroups per CU (Cout = 128, 192)
};
// The switches (plan/tile_knobs.cpp reads them; the defaults are the unset environment).  bm / occ: 0 = not forced, else the value
// given, or -1 for a value that reads as 0: any setting forbids the chain and the 32-row choice, whatever it says.
struct ConvKnobs {
  long wgs = 256;      // DHW_CONV_WGS: workgroups that fill the device in one round
  int bm = 0;          // DHW_CONV_BM
  int occ = 0;         // DHW_CONV_OCC
  int pp = 0;          // DHW_CONV_PP: bit 0 = enc1-type tall tiles, bit 1 = dec1-type, with their row halves one phase apart
  bool asym = true;    // DHW_CONV_ASYM
  bool tight = true;   // DHW_CONV_TIGHT
  bool rt = false;     // DHW_CONV_RT: A/B, force the run-time-width variants
};

// The reference's encoder blocks (model.py:85-89): Cout 128 <- 128, 192 <- 128, 256 <- 192; these input widths are compiled in.
constexpr int enc_cin(int CO) { return CO == 256 ? 192 : 128; }

constexpr long conv_tiles(const ConvShape& s, int rows) { return (long)s.B * ((s.L + rows - 1) / rows); }
// 46-row tiles for the widest blocks (L/4 level) when the 62-row tiling leaves CUs idle and the finer one still fits one round
constexpr bool conv_use_bm48(const ConvShape& s, const ConvKnobs& k) {
  if (k.bm) return k.bm == 48;
  return conv_tiles(s, 62) < k.wgs && conv_tiles(s, 46) <= k.wgs && conv_tiles(s, 46) > conv_tiles(s, 62);
}
// 32-row tiles with conv1 over 48 rows (TIGHT = 2) for the widest blocks when they fill the CUs in one round where the 46-row
// tiling leaves some idle (B = 64 at L / 4 = 122: 256 instead of 192 workgroups)
constexpr bool conv_use_asym32(const ConvShape& s, const ConvKnobs& k) {
  return k.asym && !k.bm && conv_tiles(s, 32) <= k.wgs && conv_tiles(s, 32) > conv_tiles(s, 46);
}
// BM - 4 output rows per tile where that needs no more tiles than BM - 2: the input stage then has no partial row tile
constexpr bool conv_tight(const ConvShape& s, const ConvKnobs& k, int bm) { return k.tight && (s.L + bm - 5) / (bm - 4) == (s.L + bm - 3) / (bm - 2); }

// The row of CONV_VARIANTS a launch of this shape runs under these knobs, or -1 (no compiled variant serves it).
constexpr int conv_plan(const ConvShape& s, const ConvKnobs& k) {
  if (s.f32) return s.up || s.chain ? -1 : conv_find({1, 32, s.Cout, 4, 1, 0, 0, 0, 0, 0});
  const auto pick = [&](int BM, int OCC, int UPC, int CIN, int TIGHT, int PP) { return conv_find({0, BM, s.Cout, 8, OCC, UPC, s.chain, CIN, TIGHT, PP}); };
  // 126-row tiles keep a full-resolution grid within one round of workgroups (one 8-wave workgroup per CU)
  const bool big = conv_tiles(s, 62) > k.wgs && s.tall_fits;
  if (s.chain) {   // the encoder-side blocks in front of an EncoderLayer (enc2 -> enc3, enc4 -> enc5); never under a forced tile
    if (s.up || k.bm || k.occ || (s.Cout != 192 && s.Cout != 256) || s.Cin != enc_cin(s.Cout)) return -1;
    if (s.Cout == 192) return pick(64, 1, 0, 128, 0, 0);
    return conv_use_asym32(s, k) ? pick(32, 1, 0, 192, 2, 0) : pick(conv_use_bm48(s, k) ? 48 : 64, 1, 0, 192, 0, 0);
  }
  if (s.up) {
    if (s.Cout == 128 && s.Cin == 192 && s.up_cin == 128)
      return big ? pick(128, 1, 192, 192, conv_tight(s, k, 128), (k.pp & 2) != 0) : pick(64, 1, 192, 192, 0, 0);
    if (s.Cout == 192 && s.Cin == 256 && s.up_cin == 192) return pick(64, 1, 256, 256, 0, 0);
    if (s.Cout == 256 && s.Cin == 384 && s.up_cin == 256) {
      if (conv_use_asym32(s, k)) return pick(32, 1, 384, 384, 2, 0);
      return conv_use_bm48(s, k) ? pick(48, 1, 384, 384, conv_tight(s, k, 48), 0) : pick(64, 1, 384, 384, 0, 0);
    }
    return -1;
  }
  const bool sk = !k.rt && s.Cin == enc_cin(s.Cout);   // an encoder block: static contraction lengths
  const int cin = sk ? s.Cin : 0;
  switch (s.Cout) {
    case 128:
      if (k.occ == 2 && sk && s.occ2_fits) return pick(64, 2, 0, 128, 0, 0);
      return big && k.bm != 64 ? pick(128, 1, 0, cin, 0, sk && (k.pp & 1)) : pick(64, 1, 0, cin, 0, 0);
    case 192:
      return pick(64, k.occ == 2 && sk && s.occ2_fits ? 2 : 1, 0, cin, 0, 0);
    case 256:   // (30-row tiles = 2.5x the workgroups at the L/4 level measured slower: 34.1 vs 30.8 us; DHW_CONV_BM=32 to retry)
      if (sk && conv_use_asym32(s, k)) return pick(32, 1, 0, 192, 2, 0);
      if (conv_use_bm48(s, k)) return pick(48, 1, 0, cin, 0, 0);
      return k.bm == 32 ? pick(32, 1, 0, 0, 0, 0) : pick(64, 1, 0, cin, 0, 0);
  }
  return -1;
}

// ---------------------------------------------------------------- EncoderLayer
struct EncKnobs {
  int bm = 0;        // DHW_ENC_BM192 / 256 / 384 for the layer's width, else DHW_ENC_BM: forced row tile (experiments only)
  long wgs = 256;    // DHW_ENC_WGS: smallest tile count that still gives every CU a workgroup
};
// Row tile of a (precision, width) layer at B samples of Lk rows: 64 rows when that still gives every CU a workgroup, else 32, else
// 16 (twice / four times the workgroups).  fit[i]: fits() of ENC_VARIANTS[i] (enclayer.hip); a row tile the table lacks does not fit.
inline int enc_plan_bm(bool f32, int DM, int B, int Lk, int bm_min, const EncKnobs& k, const bool* fit) {
  int bm = 64;
  if ((long)B * ((Lk + 63) / 64) < k.wgs) bm = 32;
  if (DM % 128 == 0 && (long)B * ((Lk + 31) / 32) < k.wgs) bm = 16;   // (the 4x2 wave layout of DM=192 needs >= 32 rows)
  if (k.bm) bm = k.bm;
  // LDS budget (160 KiB) of both halves: shrink the row tile until the combination fits (fp32 tiles are twice as wide)
  auto ok = [&](int m) { const int i = enc_find({f32, DM, m}); return i >= 0 && fit[i]; };
  while (bm > 16 && !ok(bm)) bm /= 2;
  if (DM % 128 != 0 && bm < 32) bm = 32;
  if (bm < bm_min) bm = bm_min;
  return bm == 16 || bm == 32 ? bm : 64;
}

// ---------------------------------------------------------------- the switches (plan/tile_knobs.cpp: the one place that reads them)
// DHW_CONV_WGS / BM / OCC / PP and the DHW_ENC_* ones are read at every call (capture time under graph replay: a test flips them
// between two handles); DHW_CONV_ASYM / TIGHT / RT once per process, by the first call of conv_knobs().
ConvKnobs conv_knobs();
int conv_stagger(int dflt);   // DHW_CONV_STAGGER, else dflt (ConvBlockParams.stagger)
EncKnobs enc_knobs(int DM);

// ---------------------------------------------------------------- queries for include/dhw_debug.h (convblock.hip / enclayer.hip, uniform build)
// conv_plan of a shape with its LDS facts filled in (up_cin = 0: no fused input stage); enc_plan_bm with enclayer.hip's fits();
// fits() and the chain modes of has_chain() (bit 0 = mode 1, bit 1 = mode 2) of ENC_VARIANTS[i]
int convblock_plan(int prec, int B, int L, int Cin, int Cout, int up_cin, bool chain, const ConvKnobs& k);
int enclayer_plan_bm(int prec, int d, int B, int Lk, int bm_min, const EncKnobs& k);
void enclayer_variant_facts(int i, int* fits, int* chain_modes);
