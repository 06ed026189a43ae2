// plan/tile_knobs.cpp — the one place that reads the tile switches of the stroke kernels from the environment (tile_plan.h says
// what each means, DESIGN 45 when each is read).  Compiled once into the library: the uniform, ragged and store-policy builds of
// convblock.hip / enclayer.hip all ask here, so the once-per-process switches are frozen once for all three.
#include <cstdlib>

#include "tile_plan.h"

namespace {
// a forced value: 0 = not set, the number given, or -1 where that reads as 0 (set, but selecting nothing)
int forced(const char* name) {
  const char* e = getenv(name);
  if (!e) return 0;
  const int v = atoi(e);
  return v ? v : -1;
}
bool frozen_flag(const char* name, bool dflt) {   // unset = dflt, else "is not 0"
  const char* e = getenv(name);
  return e ? atoi(e) != 0 : dflt;
}
}  // namespace

ConvKnobs conv_knobs() {
  static const bool asym = frozen_flag("DHW_CONV_ASYM", true), tight = frozen_flag("DHW_CONV_TIGHT", true), rt = frozen_flag("DHW_CONV_RT", false);
  ConvKnobs k;
  if (const char* e = getenv("DHW_CONV_WGS")) k.wgs = atol(e);
  k.bm = forced("DHW_CONV_BM");
  k.occ = forced("DHW_CONV_OCC");
  if (const char* e = getenv("DHW_CONV_PP")) k.pp = atoi(e);
  k.asym = asym;
  k.tight = tight;
  k.rt = rt;
  return k;
}

int conv_stagger(int dflt) {
  const char* e = getenv("DHW_CONV_STAGGER");
  return e ? atoi(e) : dflt;
}

EncKnobs enc_knobs(int DM) {
  EncKnobs k;
  const char* e = getenv(DM == 384 ? "DHW_ENC_BM384" : DM == 256 ? "DHW_ENC_BM256" : "DHW_ENC_BM192");
  if (!e) e = getenv("DHW_ENC_BM");
  if (e) k.bm = atoi(e);
  if (const char* t = getenv("DHW_ENC_WGS")) k.wgs = atol(t);
  return k;
}
