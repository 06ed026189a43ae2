// pairs.h — pairwise statistics of two sets of pooled feature vectors in double precision (include/dhw.h: dhw_pairs_pool,
// dhw_pairs_workspace_bytes, dhw_pairs_knn, dhw_pairs_cover, dhw_pairs_polysum): the ranges, the workspace layout, the number of
// column splits and every argument rule, decided without a device, and the launchers of pairs.hip.  Shared by pairs.hip and
// dhw_pairs_api.cpp.  Definition of the results: include/dhw.h and DESIGN.md §38.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../moments/moments.h"

constexpr int PAIRS_MAX_N = 16384;     // rows per set
constexpr int PAIRS_MIN_D = MOMENTS_MIN_D;
constexpr int PAIRS_MAX_D = MOMENTS_MAX_D;
constexpr int PAIRS_MAX_K = 8;         // neighbours kept per row
constexpr int PAIRS_BLOCK = 64;        // one workgroup walks 64 rows x 64 columns at a time: 4 waves of 2 x 2 tiles each
constexpr int PAIRS_THREADS = 256;
constexpr int PAIRS_MAX_SPLIT = 32;    // column splits a call may use (the partial results are sized for it)
constexpr int PAIRS_FILL = 512;        // workgroups the automatic split aims for (two per CU)

inline int pairs_pad(int n) { return (n + PAIRS_BLOCK - 1) / PAIRS_BLOCK * PAIRS_BLOCK; }

inline bool pairs_dims_ok(int M, int N, int D) {
  return M >= 1 && M <= PAIRS_MAX_N && N >= 1 && N <= PAIRS_MAX_N && D >= PAIRS_MIN_D && D <= PAIRS_MAX_D && D % MOMENTS_TILE == 0;
}

// the most column splits a call over N columns can use: one per 64 columns, at most PAIRS_MAX_SPLIT
inline int pairs_max_splits(int N) {
  const int chunks = pairs_pad(N) / PAIRS_BLOCK;
  return chunks < PAIRS_MAX_SPLIT ? chunks : PAIRS_MAX_SPLIT;
}

// column splits of a call with M rows and N columns: `forced` (DHW_PAIRS_SPLIT) when positive, else enough for PAIRS_FILL workgroups
inline int pairs_splits(int M, int N, int forced) {
  const int row_blocks = pairs_pad(M) / PAIRS_BLOCK, most = pairs_max_splits(N);
  int s = forced > 0 ? forced : (PAIRS_FILL + row_blocks - 1) / row_blocks;
  return s < 1 ? 1 : s > most ? most : s;
}

// The workspace, in doubles.  Mp / Np: M / N rounded up to 64.
//   xt  [D][Mp]   the row set, k-major, zero in the columns at or past M
//   yt  [D][Np]   the column set likewise (dhw_pairs_knn: unused, both operands are xt)
//   sqx [Mp], sqy [Np]   squared norms, zero at or past M / N
//   part          the splits' partial results: at most Mp x PAIRS_MAX_SPLIT x PAIRS_MAX_K doubles (the k candidates; count / min /
//                 argmin and the partial cube sums are smaller)
struct PairsLayout {
  int Mp, Np;
  size_t xt, yt, sqx, sqy, part, total;   // offsets and the total, in doubles
};

inline PairsLayout pairs_layout(int M, int N, int D) {
  PairsLayout l;
  l.Mp = pairs_pad(M);
  l.Np = pairs_pad(N);
  l.xt = 0;
  l.yt = l.xt + (size_t)D * l.Mp;
  l.sqx = l.yt + (size_t)D * l.Np;
  l.sqy = l.sqx + l.Mp;
  l.part = l.sqy + l.Np;
  l.total = l.part + (size_t)l.Mp * pairs_max_splits(N) * PAIRS_MAX_K;
  return l;
}

inline size_t pairs_workspace_bytes(int M, int N, int D) { return pairs_dims_ok(M, N, D) ? pairs_layout(M, N, D).total * sizeof(double) : 0; }

// ---------------------------------------------------------------- argument rules: 0, or -1 with the offending argument named in msg
#define PAIRS_FAIL(...) do { snprintf(msg, msg_len, __VA_ARGS__); return -1; } while (0)

inline int pairs_check_rows(const char* name, int n, char* msg, size_t msg_len) {
  if (n < 1 || n > PAIRS_MAX_N) PAIRS_FAIL("%s must be in [1, %d] (got %d)", name, PAIRS_MAX_N, n);
  return 0;
}

inline int pairs_check_D(int D, char* msg, size_t msg_len) {
  if (D < PAIRS_MIN_D || D > PAIRS_MAX_D || D % MOMENTS_TILE)
    PAIRS_FAIL("D must be a multiple of %d in [%d, %d] (got %d)", MOMENTS_TILE, PAIRS_MIN_D, PAIRS_MAX_D, D);
  return 0;
}

// a pointer that must be given (or may be NULL when optional) and 16-byte aligned; never dereferenced
inline int pairs_check_ptr(const char* name, const void* p, bool optional, char* msg, size_t msg_len) {
  if (!p && !optional) PAIRS_FAIL("%s is NULL", name);
  if ((uintptr_t)p & 15) PAIRS_FAIL("%s must be 16-byte aligned", name);
  return 0;
}

inline int pairs_check_ws(const void* ws, size_t ws_bytes, int M, int N, int D, char* msg, size_t msg_len) {
  const size_t need = pairs_workspace_bytes(M, N, D);
  if (ws_bytes < need) PAIRS_FAIL("ws_bytes %zu < dhw_pairs_workspace_bytes(%d, %d, %d) = %zu", ws_bytes, M, N, D, need);
  return pairs_check_ptr("ws", ws, false, msg, msg_len);
}

inline int pairs_check_pool(const void* feat, int N, int S, int D, const void* out, char* msg, size_t msg_len) {
  if (pairs_check_rows("N", N, msg, msg_len)) return -1;
  if (S < 1 || S > MOMENTS_MAX_S) PAIRS_FAIL("S must be in [1, %d] (got %d)", MOMENTS_MAX_S, S);
  if (pairs_check_D(D, msg, msg_len)) return -1;
  if ((long long)N * S * D >= (1ll << 31)) PAIRS_FAIL("N S D must stay below 2^31 (got N %d, S %d, D %d)", N, S, D);
  if (pairs_check_ptr("feat", feat, false, msg, msg_len) || pairs_check_ptr("out", out, false, msg, msg_len)) return -1;
  return 0;
}

inline int pairs_check_knn(const void* x, int N, int D, int k, const void* radius2, const void* ws, size_t ws_bytes, char* msg, size_t msg_len) {
  if (pairs_check_rows("N", N, msg, msg_len) || pairs_check_D(D, msg, msg_len)) return -1;
  if (k < 1 || k > PAIRS_MAX_K || k >= N) PAIRS_FAIL("k must be in [1, %d] and below N = %d (got %d)", PAIRS_MAX_K, N, k);
  if (pairs_check_ptr("x", x, false, msg, msg_len) || pairs_check_ptr("radius2", radius2, false, msg, msg_len)) return -1;
  return pairs_check_ws(ws, ws_bytes, N, N, D, msg, msg_len);
}

inline int pairs_check_cover(const void* q, int M, const void* ref, int N, int D, const void* radius2, const void* count, const void* nearest2,
                             const void* nearest_idx, const void* ws, size_t ws_bytes, char* msg, size_t msg_len) {
  if (pairs_check_rows("M", M, msg, msg_len) || pairs_check_rows("N", N, msg, msg_len) || pairs_check_D(D, msg, msg_len)) return -1;
  if (!radius2 != !count) PAIRS_FAIL("radius2 and count must both be given or both be NULL (%s is NULL)", radius2 ? "count" : "radius2");
  if (pairs_check_ptr("q", q, false, msg, msg_len) || pairs_check_ptr("ref", ref, false, msg, msg_len) ||
      pairs_check_ptr("radius2", radius2, true, msg, msg_len) || pairs_check_ptr("count", count, true, msg, msg_len) ||
      pairs_check_ptr("nearest2", nearest2, false, msg, msg_len) || pairs_check_ptr("nearest_idx", nearest_idx, true, msg, msg_len))
    return -1;
  return pairs_check_ws(ws, ws_bytes, M, N, D, msg, msg_len);
}

inline int pairs_check_polysum(const void* x, int M, const void* y, int N, int D, int skip_diag, const void* out, const void* ws, size_t ws_bytes,
                               char* msg, size_t msg_len) {
  if (pairs_check_rows("M", M, msg, msg_len) || pairs_check_rows("N", N, msg, msg_len) || pairs_check_D(D, msg, msg_len)) return -1;
  if (skip_diag && M != N) PAIRS_FAIL("skip_diag needs M == N (got M %d, N %d)", M, N);
  if (pairs_check_ptr("x", x, false, msg, msg_len) || pairs_check_ptr("y", y, false, msg, msg_len) || pairs_check_ptr("out", out, false, msg, msg_len))
    return -1;
  return pairs_check_ws(ws, ws_bytes, M, N, D, msg, msg_len);
}

#undef PAIRS_FAIL

// ---------------------------------------------------------------- launchers (pairs.hip): no allocation, no synchronisation
// ws holds pairs_layout(...) doubles; splits = pairs_splits(...)
hipError_t launch_pairs_knn(const double* x, int N, int D, int k, double* radius2, double* ws, int splits, hipStream_t st);
hipError_t launch_pairs_cover(const double* q, int M, const double* ref, int N, int D, const double* radius2, int* count, double* nearest2,
                              int* nearest_idx, double* ws, int splits, hipStream_t st);
hipError_t launch_pairs_polysum(const double* x, int M, const double* y, int N, int D, int skip_diag, double* out, double* ws, int splits,
                                hipStream_t st);
