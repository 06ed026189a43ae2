// attnmap.hip — the probabilities of one cross attention, written out (include/dhw.h: dhw_attention).  The
// fused EncoderLayer kernels keep them in registers (attn_core.h); this kernel recomputes them from the stored Q and K.
//
// One workgroup per (sample, 16 query rows), one wave per head.  In a wave, lane = 4 * row + c: the lane holds its row's 64
// query values in registers (fp32) and owns the keys c, c + 4, ...  Plain FMA on values converted to fp32: the whole map is
// ~90 MFLOP at B = 64, L = 488, Lt = 30, so the kernel is bound by its launch and by load latency, not by arithmetic, and a
// k-ordered fmaf chain gives sums whose order depends on nothing but the row itself (a ragged row equals its alone run).
#include "attnmap.h"

#include "../dhw_common.h"
#include "../dhw_kernels.h"

namespace {

// 8 consecutive elements from a 16-byte aligned address, as fp32
DHW_DEV void load8(const bf16_t* p, float (&v)[8]) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
  v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
  v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}
DHW_DEV void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}

// argmax bookkeeping: the larger value wins, equal values go to the lower index
DHW_DEV void take_better(float& best, int& bi, float v, int i) {
  if (v > best || (v == best && i < bi)) { best = v; bi = i; }
}

template <typename T, int H>
__global__ __launch_bounds__(64 * H) void attnmap_kernel(const AttnMapParams p) {
  extern __shared__ __attribute__((aligned(16))) float am_tile[];   // [H][16][ltp]: logits, then exponentials, then probabilities
  const int tid = threadIdx.x, h = tid >> 6, lane = tid & 63, r = lane >> 2, c = lane & 3;
  const int b = blockIdx.y, q0 = blockIdx.x * ATTNMAP_ROWS;
  const int Lq = p.Lq, Lt = p.Lt, ltp = (Lt + 3) & ~3;
  const int nq = p.lens ? min(p.lens[b] >> p.lsh, Lq) : Lq;   // this sample's query rows
  const int nr = min(ATTNMAP_ROWS, Lq - q0);                   // rows of the tile that exist in the outputs (grid: q0 < Lq)
  if (q0 >= nq) {   // the whole tile lies past the sample's end: zeros and -1, nothing is read
    if (p.probs) {
      float* o = p.probs + (((long)b * H + h) * Lq + q0) * Lt;
      for (int i = lane; i < nr * Lt; i += 64) o[i] = 0.f;
    }
    if (h == 0) {
      if (p.mean) {
        float* o = p.mean + ((long)b * Lq + q0) * Lt;
        for (int i = lane; i < nr * Lt; i += 64) o[i] = 0.f;
      }
      if (p.token && lane < nr) p.token[(long)b * Lq + q0 + lane] = -1;
    }
    return;
  }
  const int q = q0 + r;
  const bool valid = q < nq;            // a row of the sample
  const bool exists = q < Lq;           // a row of the outputs (past the sample's end: zeros and -1)
  const int qc = valid ? q : nq - 1;    // lanes without a row of their own work on the sample's last one: every load stays inside the sample
  float qv[ATTNMAP_D];
  {
    const T* qp = reinterpret_cast<const T*>(p.Q) + ((long)b * Lq + qc) * p.ldq + h * ATTNMAP_D;
#pragma unroll
    for (int j = 0; j < ATTNMAP_D / 8; ++j) {
      float v[8];
      load8(qp + 8 * j, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) qv[8 * j + i] = v[i];
    }
  }
  float* row = am_tile + ((long)h * ATTNMAP_ROWS + r) * ltp;
  const T* kb = reinterpret_cast<const T*>(p.K) + (long)b * Lt * p.ldk + h * ATTNMAP_D;
  const int64_t* tx = p.text + (long)b * Lt;
  float mx = -INFINITY;
  for (int k = c; k < Lt; k += 4) {
    const T* kp = kb + (long)k * p.ldk;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < ATTNMAP_D / 8; ++j) {
      float v[8];
      load8(kp + 8 * j, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = fmaf(qv[8 * j + i], v[i], acc);
    }
    const float s = acc * 0.125f + (tx[k] == 0 ? -1e9f : 0.f);
    row[k] = s;
    mx = fmaxf(mx, s);
  }
  // the row's 4 lanes: max, then the sum of the exponentials (each lane its keys in order, then (c0 + c1) + (c2 + c3))
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  float sum = 0.f;
  for (int k = c; k < Lt; k += 4) {
    const float e = expf(row[k] - mx);
    row[k] = e;
    sum += e;
  }
  sum += __shfl_xor(sum, 1, 64);
  sum += __shfl_xor(sum, 2, 64);
  float* po = p.probs ? p.probs + (((long)b * H + h) * Lq + (exists ? q : 0)) * Lt : nullptr;
  for (int k = c; k < Lt; k += 4) {
    const float v = row[k] / sum;
    row[k] = v;
    if (po && exists) po[k] = valid ? v : 0.f;
  }
  __syncthreads();
  if (h != 0) return;
  // wave 0: the mean over heads in head order, times 1/H, and the first argmax of it
  const float inv = 1.0f / (float)H;
  const float* t0 = am_tile + (long)r * ltp;
  const long hs = (long)ATTNMAP_ROWS * ltp;   // head stride of the tile
  float* mo = p.mean ? p.mean + ((long)b * Lq + (exists ? q : 0)) * Lt : nullptr;
  float best = -INFINITY;
  int bi = 0;   // nothing compares greater than -inf only when every value is NaN: such a row gets token 0, an index like any other
  if ((Lt & 3) == 0) {
    for (int k = 4 * c; k < Lt; k += 16) {
      f32x4 a = *reinterpret_cast<const f32x4*>(t0 + k);
#pragma unroll
      for (int hh = 1; hh < H; ++hh) a += *reinterpret_cast<const f32x4*>(t0 + hh * hs + k);
      a *= inv;
      if (mo && exists) *reinterpret_cast<f32x4*>(mo + k) = valid ? a : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) take_better(best, bi, a[i], k + i);
    }
  } else {
    for (int k = c; k < Lt; k += 4) {
      float a = t0[k];
#pragma unroll
      for (int hh = 1; hh < H; ++hh) a += t0[hh * hs + k];
      a *= inv;
      if (mo && exists) mo[k] = valid ? a : 0.f;
      take_better(best, bi, a, k);
    }
  }
#pragma unroll
  for (int m = 1; m <= 2; m <<= 1) {
    const float ob = __shfl_xor(best, m, 64);
    const int oi = __shfl_xor(bi, m, 64);
    take_better(best, bi, ob, oi);
  }
  if (p.token && c == 0 && exists) p.token[(long)b * Lq + q] = valid ? bi : -1;
}

template <typename T, int H>
hipError_t launch_h(const AttnMapParams& p, hipStream_t st) {
  const int ltp = (p.Lt + 3) & ~3;
  const size_t lds = (size_t)H * ATTNMAP_ROWS * ltp * sizeof(float);   // at most 63 KiB (ATTNMAP_MAX_LT): the default limit holds it
  hipLaunchKernelGGL((attnmap_kernel<T, H>), dim3((unsigned)((p.Lq + ATTNMAP_ROWS - 1) / ATTNMAP_ROWS), (unsigned)p.B), dim3(64 * H), lds, st, p);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_t(const AttnMapParams& p, hipStream_t st) {
  switch (p.H) {
    case 3: return launch_h<T, 3>(p, st);
    case 4: return launch_h<T, 4>(p, st);
    case 6: return launch_h<T, 6>(p, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_attnmap(int prec, const AttnMapParams& p, hipStream_t st) {
  if (!p.Q || !p.K || !p.text || p.B < 1 || p.Lq < 1 || p.Lt < 1 || p.Lt > ATTNMAP_MAX_LT || (!p.probs && !p.mean && !p.token)) return hipErrorInvalidValue;
  if (p.ldq < p.H * ATTNMAP_D || p.ldk < p.H * ATTNMAP_D || (p.ldq & 7) || (p.ldk & 7)) return hipErrorInvalidValue;
  if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.mean) & 15) return hipErrorInvalidValue;
  return prec == PREC_BF16 ? launch_t<bf16_t>(p, st) : launch_t<float>(p, st);
}
