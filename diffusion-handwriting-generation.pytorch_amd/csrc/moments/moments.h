// moments.h — feature moments (include/dhw.h: dhw_moments_workspace_bytes, dhw_moments_update): the ranges, the workspace size
// and every argument rule, decided without a device, and the launcher of moments.hip.  Shared by moments.hip and
// dhw_moments_api.cpp.  Definition of the result: include/dhw.h and DESIGN.md §37.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>

constexpr int MOMENTS_MAX_N = 16384;   // samples per call (quality.py chunks a longer batch)
constexpr int MOMENTS_MAX_S = 64;      // positions pooled per sample
constexpr int MOMENTS_MIN_D = 16;      // one MFMA tile
constexpr int MOMENTS_MAX_D = 2048;
constexpr int MOMENTS_TILE = 16;       // v_mfma_f64_16x16x4_f64: D is a multiple of this
constexpr int MOMENTS_BLOCK = 64;      // one workgroup owns a 64 x 64 block of gram: 4 waves of 2 x 2 tiles each
constexpr int MOMENTS_THREADS = 256;

inline bool moments_dims_ok(int N, int S, int D) {
  return N >= 1 && N <= MOMENTS_MAX_N && S >= 1 && S <= MOMENTS_MAX_S && D >= MOMENTS_MIN_D && D <= MOMENTS_MAX_D && D % MOMENTS_TILE == 0 &&
         (long long)N * S * D < (1ll << 31);
}

// the pooled matrix p, f64 [N,D]
inline size_t moments_workspace_bytes(int N, int S, int D) { return moments_dims_ok(N, S, D) ? (size_t)N * D * sizeof(double) : 0; }

// Every argument rule of dhw_moments_update: 0 on success, else -1 with the offending argument named in msg.  Pointers are
// only compared and never dereferenced.
inline int moments_check_args(const void* feat, int N, int S, int D, const void* sum, const void* gram, const void* ws, size_t ws_bytes,
                              char* msg, size_t msg_len) {
  if (N < 1 || N > MOMENTS_MAX_N) { snprintf(msg, msg_len, "N must be in [1, %d] (got %d)", MOMENTS_MAX_N, N); return -1; }
  if (S < 1 || S > MOMENTS_MAX_S) { snprintf(msg, msg_len, "S must be in [1, %d] (got %d)", MOMENTS_MAX_S, S); return -1; }
  if (D < MOMENTS_MIN_D || D > MOMENTS_MAX_D || D % MOMENTS_TILE) {
    snprintf(msg, msg_len, "D must be a multiple of %d in [%d, %d] (got %d)", MOMENTS_TILE, MOMENTS_MIN_D, MOMENTS_MAX_D, D);
    return -1;
  }
  if ((long long)N * S * D >= (1ll << 31)) { snprintf(msg, msg_len, "N S D must stay below 2^31 (got N %d, S %d, D %d)", N, S, D); return -1; }
  if (!feat) { snprintf(msg, msg_len, "feat is NULL"); return -1; }
  if (!sum) { snprintf(msg, msg_len, "sum is NULL"); return -1; }
  if (!gram) { snprintf(msg, msg_len, "gram is NULL"); return -1; }
  if ((uintptr_t)feat & 15) { snprintf(msg, msg_len, "feat must be 16-byte aligned"); return -1; }
  if ((uintptr_t)sum & 15) { snprintf(msg, msg_len, "sum must be 16-byte aligned"); return -1; }
  if ((uintptr_t)gram & 15) { snprintf(msg, msg_len, "gram must be 16-byte aligned"); return -1; }
  const size_t need = moments_workspace_bytes(N, S, D);
  if (ws_bytes < need) { snprintf(msg, msg_len, "ws_bytes %zu < dhw_moments_workspace_bytes(%d, %d, %d) = %zu", ws_bytes, N, S, D, need); return -1; }
  if (need && !ws) { snprintf(msg, msg_len, "ws is NULL"); return -1; }
  if ((uintptr_t)ws & 15) { snprintf(msg, msg_len, "ws must be 16-byte aligned"); return -1; }
  return 0;
}

// rule 1 alone: pooled[n][d] = (sum_s (double)feat[n][s][d]) / S, s ascending (moments_pool_kernel; also behind dhw_pairs_pool)
hipError_t launch_moments_pool(const float* feat, int N, int S, int D, double* pooled, hipStream_t st);

// pooled = ws, f64 [N,D]: three launches on st (pool, column sums, gram), no allocation, no synchronisation
hipError_t launch_moments(const float* feat, int N, int S, int D, double* sum, double* gram, double* pooled, hipStream_t st);
