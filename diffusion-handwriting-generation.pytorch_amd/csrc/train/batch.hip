// batch.hip — the training batch of one update, drawn and gathered on the device from a dataset resident in HBM
// (reference: next(iter(train_loader)) train.py:98, get_alphas utils/nn.py:42-61, the style-source rule dataset.py:110-115).
//
// batch_draw_kernel: ONE Philox4x32-10 block per batch sample (philox_round of heads_core.h, normal2's key schedule):
//   key = rng[0] (the seed), counter = (lo, hi of the 64-bit stream rng[1] * B + b, 0, 0).  c3 = 0 is the batch draw's own
//   lane of the generator: eps uses 1, the style mask 2, the dropout sites 3 and up (train.hip).  Of the output words w0..w3:
//     idx[b]    = (uint64(w0) * N) >> 32                       a sample in [0, N), with replacement
//     i         = (uint64(w1) * (T - 1)) >> 32                 a schedule interval
//     u         = ((w2 >> 8) + 0.5f) * 2^-24
//     alphas[b] = u * (abar[i + 1] - abar[i]) + abar[i]        three separately rounded fp32 operations (no fma)
//     sigma[b]  = sqrt(alphas[b])                              correctly rounded
//     style_src = idx without group tables or in a group of one; else with s = grp_size[idx]:
//                 r = (uint64(w3) * (s - 1)) >> 32, j = r + (r >= grp_pos[idx]), style_src = members[grp_start[idx] + j]
//                 — uniform over the OTHER lines of the same writer.
//   The multiply-high mapping of a 32-bit word onto [0, n) is biased by at most n / 2^32 (some values are hit
//   ceil(2^32 / n) times, the others floor(2^32 / n) times): < 2^-11 for the 0.1 M lines of IAM, nothing for T - 1 = 59.
//
// batch_gather_kernel: rows idx[b] of strokes / text and row style_src[b] of style into the step's static input buffers, one
//   16-byte piece (style, strokes) or one token (text) per thread; the grid covers all B rows at once.
#include "../heads_core.h"
#include "train_common.h"

using namespace dhw_train;

namespace {

DHW_DEV uint4 keep_if(bool k, const uint4& v) { return make_uint4(k ? v.x : 0u, k ? v.y : 0u, k ? v.z : 0u, k ? v.w : 0u); }   // (a select per word, no indexing)

__global__ __launch_bounds__(256) void batch_draw_kernel(const uint64_t* rng, int N, int B, const float* abar, int T, const int* grp_start, const int* grp_size,
                                                         const int* grp_pos, const int* members, int* idx, int* style_src, float* alphas, float* sigma) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint64_t seed = rng[0], stream = rng[1] * (uint64_t)B + (uint64_t)b;
  uint32_t c0 = (uint32_t)stream, c1 = (uint32_t)(stream >> 32), c2 = 0u, c3 = 0u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const int id = (int)(((uint64_t)c0 * (uint32_t)N) >> 32);
  const int i = (int)(((uint64_t)c1 * (uint32_t)(T - 1)) >> 32);
  float a;
  {
    // sub, mul, add each rounded on its own, so that numpy reproduces the bits.  (__fmul_rn / __fadd_rn are plain * and + in this
    // toolchain and contract into an fma once inlined; the pragma governs the operators written in this block.)
#pragma clang fp contract(off)
    const float u = ((float)(c2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float lo = abar[i];
    const float d = abar[i + 1] - lo;
    const float ud = u * d;
    a = ud + lo;
  }
  int src = id;
  if (grp_start) {
    const int s = grp_size[id];
    if (s > 1) {
      const int r = (int)(((uint64_t)c3 * (uint32_t)(s - 1)) >> 32);
      src = members[grp_start[id] + r + (r >= grp_pos[id] ? 1 : 0)];
    }
  }
  idx[b] = id;
  style_src[b] = src;
  alphas[b] = a;
  sigma[b] = sqrtf(a);   // the IEEE square root (hipcc's default for sqrtf; __fsqrt_rn is the 1-ulp native one in this build)
}

// Work of one sample, in 16-byte pieces / tokens: [0, nsty) the style row, [nsty, nsty + nstk) groups of 4 stroke points (48 bytes in,
// 32 + 16 out), then Lt tokens.  Consecutive lanes take consecutive pieces.  A sample whose idx or style_src lies outside [0, N) reads
// row 0 (never the index) and writes zeros with mask = 1: loads stay unconditional, the zero is a select.
__global__ __launch_bounds__(256) void batch_gather_kernel(const float* strokes, const int64_t* text, const float* style, const int* idx, const int* style_src, int N,
                                                           int L, int Lt, int nsty, int bps, float* x, float* pen, int64_t* ids, float* mask, float* style_out) {
  const int b = blockIdx.x / bps;
  int p = (blockIdx.x % bps) * 256 + threadIdx.x;
  const int ri = idx[b], rs = style_src[b];
  const bool ok = (unsigned)ri < (unsigned)N && (unsigned)rs < (unsigned)N;
  const long row = ok ? ri : 0, srow = ok ? rs : 0;
  if (p < nsty) {
    const uint4 v = reinterpret_cast<const uint4*>(style)[srow * nsty + p];
    reinterpret_cast<uint4*>(style_out)[(long)b * nsty + p] = keep_if(ok, v);
    return;
  }
  p -= nsty;
  const int nstk = L >> 2;
  if (p < nstk) {
    const uint4* s = reinterpret_cast<const uint4*>(strokes) + (row * nstk + p) * 3;
    const uint4 q0 = keep_if(ok, s[0]), q1 = keep_if(ok, s[1]), q2 = keep_if(ok, s[2]);   // points 4p .. 4p+3: x0 y0 p0 x1 | y1 p1 x2 y2 | p2 x3 y3 p3
    uint4* xo = reinterpret_cast<uint4*>(x) + ((long)b * nstk + p) * 2;
    xo[0] = make_uint4(q0.x, q0.y, q0.w, q1.x);
    xo[1] = make_uint4(q1.z, q1.w, q2.y, q2.z);
    reinterpret_cast<uint4*>(pen)[(long)b * nstk + p] = make_uint4(q0.z, q1.y, q2.x, q2.w);
    return;
  }
  p -= nstk;
  if (p < Lt) {
    int64_t t = text[row * Lt + p];
    if (!ok) t = 0;
    ids[(long)b * Lt + p] = t;
    mask[(long)b * Lt + p] = t == 0 ? 1.0f : 0.0f;
  }
}

}  // namespace

hipError_t launch_batch_draw(const uint64_t* rng, int N, int B, const float* abar, int T, const int* grp_start, const int* grp_size, const int* grp_pos,
                             const int* members, int* idx, int* style_src, float* alphas, float* sigma, hipStream_t st) {
  hipLaunchKernelGGL(batch_draw_kernel, dim3(nb(B)), dim3(256), 0, st, rng, N, B, abar, T, grp_start, grp_size, grp_pos, members, idx, style_src, alphas, sigma);
  return hipGetLastError();
}

hipError_t launch_batch_gather(const float* strokes, const int64_t* text, const float* style, const int* idx, const int* style_src, int N, int B, int L, int Lt,
                               int S, float* x, float* pen, int64_t* ids, float* mask, float* style_out, hipStream_t st) {
  const long nsty = (long)S * 320, per = nsty + L / 4 + Lt, bps = (per + 255) / 256;
  if (per > 0x7fffff00L || bps * B > 0x7fffffffL) return hipErrorInvalidValue;   // (piece and block numbers are ints)
  hipLaunchKernelGGL(batch_gather_kernel, dim3((unsigned)(bps * B)), dim3(256), 0, st, strokes, text, style, idx, style_src, N, L, Lt, (int)nsty, (int)bps, x, pen, ids,
                     mask, style_out);
  return hipGetLastError();
}
