// tile_plan_check.cpp — csrc/plan/tile_plan.h on its own (host compiler, AddressSanitizer + UBSan; tests/test_tile_plan_cpu.py):
// the ConvBlock plan over B 1..96 x every even row count 2..1024 for every ConvBlock role of the model, under every combination
// of the switches and of the LDS facts (main() says on which grid), in both precisions; the EncoderLayer row tile likewise.
//     tile_plan_check FITS      FITS: one '0' / '1' per row of DHW_ENC_VARIANTS, fits() as the library reports it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/plan/tile_plan.h"

#define CHECK(c)                                                                                                                       \
  do {                                                                                                                                 \
    if (!(c)) {                                                                                                                        \
      std::printf("FAILED %s (line %d): prec %d role %d B %d L %d knobs wgs %ld bm %d occ %d pp %d asym %d tight %d rt %d lds %d%d plan %d\n", #c, \
                  __LINE__, s.f32, role, s.B, s.L, k.wgs, k.bm, k.occ, k.pp, k.asym, k.tight, k.rt, s.tall_fits, s.occ2_fits, i);      \
      return 1;                                                                                                                        \
    }                                                                                                                                  \
  } while (0)

// (Cin, Cout, width of the fused input stage's skip activation or 0, chained): enc1, enc2, enc2 -> enc3.a, enc4, enc4 -> enc5.a,
// dec3 / dec2 / dec1 with the fused input stage, dec3 / dec2 / dec1 without it
struct Role { int Cin, Cout, up_cin; bool chain; };
static const Role ROLES[] = {{128, 128, 0, false}, {128, 192, 0, false}, {128, 192, 0, true}, {192, 256, 0, false}, {192, 256, 0, true}, {384, 256, 256, false},
                             {256, 192, 192, false}, {192, 128, 128, false}, {384, 256, 0, false}, {256, 192, 0, false}, {192, 128, 0, false}};

static_assert(conv_find({0, 32, 256, 8, 1, 0, 1, 192, 2, 0}) >= 0 && conv_find({0, 32, 256, 8, 1, 0, 1, 192, 1, 0}) == -1, "conv_find");
static_assert(conv_plan({false, 64, 122, 192, 256, false, 0, true, true, true}, ConvKnobs{}) == conv_find({0, 32, 256, 8, 1, 0, 1, 192, 2, 0}), "the bench shape's enc4");

// one point of the ConvBlock plan: 0 = every assertion holds
static int check_conv(int f32, const ConvKnobs& k, bool tall_fits, bool occ2_fits, int role, int B, int L) {
  const Role& r = ROLES[role];
  const ConvShape s{f32 != 0, B, L, r.Cin, r.Cout, r.up_cin != 0, r.up_cin, r.chain, tall_fits, occ2_fits};
  const int i = conv_plan(s, k);
  CHECK(i >= -1 && i < N_CONV_VARIANTS);
  const bool auto_chain = r.chain && i >= 0 && CONV_VARIANTS[i].TIGHT == 2;   // convblock_chain_auto (csrc/convblock.hip)
  if (i < 0) {   // refused: only a chain under a forced tile, or what fp32 handles never launch
    CHECK(r.chain || (f32 && r.up_cin));
    CHECK(f32 || k.bm || k.occ);
    return 0;
  }
  const ConvVariant& v = CONV_VARIANTS[i];
  CHECK(v.f32 == f32 && v.CO == r.Cout && v.NW == (f32 ? 4 : 8));
  CHECK(v.CH == r.chain && v.UPC == (r.up_cin ? r.Cin : 0) && (v.CIN == 0 || v.CIN == r.Cin));
  CHECK(!v.UPC || v.CIN == v.UPC);                                  // the fused input stage is compiled for static widths
  CHECK(!(v.CH && (k.bm || k.occ)));                                // no chain under a forced tile
  CHECK(v.OCC == 1 || (k.occ == 2 && occ2_fits && v.BM == 64));
  CHECK(v.BM <= 64 || tall_fits);
  const int rows = v.rows(), tiles = (L + rows - 1) / rows;         // (the kernels' own tile count)
  CHECK(rows > 0 && rows <= v.BM && (long)tiles * rows >= L && (long)(tiles - 1) * rows < L);
  CHECK((v.TIGHT == 2) == (v.BM == 32 && v.CIN != 0));              // the asymmetric tiles: 32 rows, static widths ...
  CHECK(v.TIGHT != 2 || (k.asym && !k.bm && (long)B * tiles <= k.wgs));   // ... only where they fill one round, never forced
  CHECK(!auto_chain || conv_use_asym32(s, k));
  CHECK(!(r.chain && r.Cout == 256 && conv_use_asym32(s, k)) || auto_chain);
  CHECK(v.TIGHT != 1 || (k.tight && (L + rows - 1) / rows == (L + rows + 1) / (rows + 2)));   // BM - 4 rows cost no tile
  CHECK(k.bm != 64 || r.up_cin || v.BM == 64);                      // DHW_CONV_BM=64 disables the tall and the 46- / 32-row choices
  CHECK(k.bm != 48 || r.Cout != 256 || v.BM == 48);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2 || (int)std::strlen(argv[1]) != N_ENC_VARIANTS) return std::printf("usage: tile_plan_check FITS (%d digits)\n", N_ENC_VARIANTS), 2;
  bool fit[N_ENC_VARIANTS];
  for (int j = 0; j < N_ENC_VARIANTS; ++j) fit[j] = argv[1][j] == '1';
  for (int a = 0; a < N_CONV_VARIANTS; ++a)   // a variant is named once
    for (int b = 0; b < a; ++b)
      if (CONV_VARIANTS[a] == CONV_VARIANTS[b]) return std::printf("FAILED: ConvBlock variant %d is variant %d again\n", a, b), 1;
  // Every combination of the switches and of the LDS facts (3072), in bf16; fp32 reads none of them.  The whole grid B 1..96 x even
  // L 2..1024 runs where at most one switch or fact leaves its default; the other combinations on a thinner grid (eight batch
  // sizes around the tiling thresholds; every even L up to 128, every sixteenth above) - the full product over the whole grid is
  // 1.7e9 points, minutes under the sanitizers.
  static const long WGS[3] = {256, 2, 128};
  static const int BM[4] = {0, 32, 48, 64};
  static const int FEW_B[8] = {1, 2, 3, 8, 32, 64, 65, 96};
  const int nroles = (int)(sizeof(ROLES) / sizeof(ROLES[0]));
  long points = 0;
  for (int f32 = 0; f32 < 2; ++f32)
    for (int kn = 0; kn < 3 * 4 * 2 * 4 * 8 * 4; ++kn) {
      ConvKnobs k;
      int q = kn, off = 0;   // off: how many switches / facts are not at their default
      k.wgs = WGS[q % 3], off += q % 3 != 0, q /= 3;
      k.bm = BM[q % 4], off += q % 4 != 0, q /= 4;
      k.occ = (q % 2) * 2, off += q % 2, q /= 2;
      k.pp = q % 4, off += q % 4 != 0, q /= 4;
      k.asym = !(q & 1), k.tight = !(q & 2), k.rt = (q & 4) != 0, off += (q & 1) + (q >> 1 & 1) + (q >> 2 & 1), q /= 8;
      const bool tall_fits = !(q & 1), occ2_fits = !(q & 2);
      off += (q & 1) + (q >> 1 & 1);
      if (f32 && kn) break;
      for (int role = 0; role < nroles; ++role)
        if (off <= 1) {
          for (int B = 1; B <= 96; ++B)
            for (int L = 2; L <= 1024; L += 2, ++points)
              if (check_conv(f32, k, tall_fits, occ2_fits, role, B, L)) return 1;
        } else {
          for (int B : FEW_B)
            for (int L = 2; L <= 1024; L += L < 128 ? 2 : 16, ++points)
              if (check_conv(f32, k, tall_fits, occ2_fits, role, B, L)) return 1;
        }
    }
  long enc_points = 0;
  for (int f32 = 0; f32 < 2; ++f32)
    for (int DM : {192, 256, 384})
      for (int bm : {0, 16, 32, 64})
        for (long wgs : {256L, 128L, 2L})
          for (int bm_min : {0, 32})   // (32: enc5 under chain mode 2, bf16 only)
            for (int B = 1; B <= 96; ++B)
              for (int Lk = 1; Lk <= 1024; ++Lk) {
                if (bm_min && (f32 || DM != 256)) continue;
                EncKnobs k;
                k.bm = bm, k.wgs = wgs;
                const int m = enc_plan_bm(f32 != 0, DM, B, Lk, bm_min, k, fit), i = enc_find({f32, DM, m});
                ++enc_points;
                if (!((m == 16 || m == 32 || m == 64) && m >= bm_min && i >= 0 && fit[i]))
                  return std::printf("FAILED EncoderLayer: prec %d d %d bm %d wgs %ld bm_min %d B %d Lk %d -> %d (row %d)\n", f32, DM, bm, wgs, bm_min, B, Lk, m, i), 1;
              }
  std::printf("ok %ld %ld\n", points, enc_points);
  return 0;
}
