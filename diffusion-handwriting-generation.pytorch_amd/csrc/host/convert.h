// host/convert.h — number formats and weight layouts shared by the three API units (sampler, StyleExtractor, training).
// Pure C++: no HIP, so tests/cpp/hostpack_check.cpp pins all of it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/dhw.h"

#pragma GCC visibility push(hidden)   // internal to libdhw_hip.so: nothing of csrc/host/ is exported

inline uint16_t f2bf(float f) {   // round-to-nearest-even; NaN stays NaN
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf2f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline float h2f(uint16_t h) {   // IEEE half -> float
  const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
  float v;
  if (e == 0) v = std::ldexp((float)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = std::ldexp((float)(m | 1024), (int)e - 25);
  return s ? -v : v;
}

// n elements of a state_dict tensor (dtype: DHW_F32 / DHW_BF16 / DHW_F16 / DHW_F64 of include/dhw.h) as fp32; false = unknown dtype
inline bool to_f32(float* dst, const void* src, int dtype, size_t n) {
  switch (dtype) {
    case DHW_F32: std::memcpy(dst, src, n * 4); return true;
    case DHW_BF16: for (size_t i = 0; i < n; ++i) dst[i] = bf2f(((const uint16_t*)src)[i]); return true;
    case DHW_F16: for (size_t i = 0; i < n; ++i) dst[i] = h2f(((const uint16_t*)src)[i]); return true;
    case DHW_F64: for (size_t i = 0; i < n; ++i) dst[i] = (float)((const double*)src)[i]; return true;
    default: return false;
  }
}

// The contract between the host and every GEMM kernel: a row-major weight matrix Wf[N][K] (N % 16 == 0, K % 32 == 0) in
// MFMA-fragment order [N/16][K/32][64 lanes][8]: lane l holds Wf[nt*16 + (l&15)][kc*32 + 8*(l>>4) + j].
inline std::vector<float> pack_mfma(const std::vector<float>& wf, int N, int K) {
  std::vector<float> pk((size_t)N * K);
  size_t o = 0;
  for (int nt = 0; nt < N / 16; ++nt)
    for (int kc = 0; kc < K / 32; ++kc)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) pk[o++] = wf[(size_t)(nt * 16 + (l & 15)) * K + kc * 32 + 8 * (l >> 4) + j];
  return pk;
}

// Conv1d weight [Cout][Cin][3] -> GEMM matrix [Cout][tap*Cin + c]
inline std::vector<float> conv_flat(const std::vector<float>& w, int cout, int cin) {
  std::vector<float> f((size_t)cout * cin * 3);
  for (int n = 0; n < cout; ++n)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < 3; ++t) f[(size_t)n * cin * 3 + t * cin + c] = w[((size_t)n * cin + c) * 3 + t];
  return f;
}

#pragma GCC visibility pop
