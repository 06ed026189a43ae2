// cond_drop.hip — conditioning dropout of a training batch (include/dhw_train.h: dhw_train_cond_drop): with
// probability p a sample loses its prompt AND its writer, so that the trained denoiser also answers the null condition that
// classifier-free guidance extrapolates away from.
//
// ONE Philox4x32-10 block per batch sample (philox_round of heads_core.h, normal2's key schedule): key = rng[0] (the seed),
// counter = (lo, hi of the 64-bit stream rng[1] * B + b, 1, 0).  Word 2 = 1 with word 3 = 0 is this draw's own lane of the
// generator: (0, 0) is the batch draw (batch.hip), word 3 = 1 eps, 2 the style mask, 3 and up the dropout sites (train.hip).
//   u = ((w0 >> 8) + 0.5f) * 2^-24,   dropped[b] = u < p.
// A dropped sample's ids row becomes [1, 0, ...] (the end token, then padding: Tokenizer().encode("")), its padding-mask row
// [0, 1, ...] (what ids == 0 gives) and its style rows 0.  Every thread of a sample evaluates the block itself; a thread owns one
// 16-byte piece of the style row or one token (a token row starts on an 8-byte boundary, a mask row on a 4-byte one).  Loads and
// stores are unconditional, the null value is a select (batch_gather_kernel's style); the grid covers all B samples at once.
#include "../heads_core.h"
#include "train_common.h"

using namespace dhw_train;

namespace {

__global__ __launch_bounds__(256) void cond_drop_kernel(const uint64_t* rng, int B, int Lt, int nsty, int bps, float p, int64_t* ids, float* mask, float* style,
                                                        int* dropped) {
  const int b = blockIdx.x / bps;
  int piece = (blockIdx.x % bps) * 256 + threadIdx.x;
  const uint64_t seed = rng[0], stream = rng[1] * (uint64_t)B + (uint64_t)b;
  uint32_t c0 = (uint32_t)stream, c1 = (uint32_t)(stream >> 32), c2 = 1u, c3 = 0u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float u = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const bool drop = u < p;
  if (piece == 0) dropped[b] = drop ? 1 : 0;
  if (piece < nsty) {
    uint4* s = reinterpret_cast<uint4*>(style) + (long)b * nsty + piece;
    const uint4 v = *s;
    *s = make_uint4(drop ? 0u : v.x, drop ? 0u : v.y, drop ? 0u : v.z, drop ? 0u : v.w);
    return;
  }
  piece -= nsty;
  if (piece < Lt) {
    const long i = (long)b * Lt + piece;
    const int64_t t = ids[i];
    const float m = mask[i];
    ids[i] = drop ? (piece == 0 ? 1 : 0) : t;
    mask[i] = drop ? (piece == 0 ? 0.0f : 1.0f) : m;
  }
}

}  // namespace

hipError_t launch_cond_drop(const uint64_t* rng, int B, int Lt, int S, float p, int64_t* ids, float* mask, float* style, int* dropped, hipStream_t st) {
  const long nsty = (long)S * 320, per = nsty + Lt, bps = (per + 255) / 256;
  if (B < 1 || Lt < 1 || S < 1 || per > 0x7fffff00L || bps * B > 0x7fffffffL) return hipErrorInvalidValue;   // (piece and block numbers are ints)
  hipLaunchKernelGGL(cond_drop_kernel, dim3((unsigned)(bps * B)), dim3(256), 0, st, rng, B, Lt, (int)nsty, (int)bps, p, ids, mask, style, dropped);
  return hipGetLastError();
}
