// paths.h — launchers of the vector twin of the page compositor (include/dhw.h: dhw_paths); shared by
// paths.hip and dhw_paths_api.cpp.  What needs no device (sizes, argument rules) is in paths_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "paths_host.h"

constexpr int PATHS_ITEMS = PATHS_MAX_L / PATHS_THREADS;   // strokes per thread (fixed: the summation order of the scan depends
                                                           // on the stroke index alone, and is the page compositor's)
static_assert(PATHS_ITEMS == 16, "the kernel keeps a thread's masks in the low 16 bits of an unsigned");

// the outputs of dhw_paths, by value
struct PathsOut {
  float4* points;     // [N,L] x (x, y, tx, ty)
  int32_t* index;     // [N,L,2]
  int32_t* counts;    // [N,2]
  float* scale;       // [1]
  float* boxes;       // [N,4]
};

// s_n of every line -> sn[N] (+inf for a line that takes no part)
hipError_t launch_paths_limits(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, const PageGeometry& g, float* sn,
                               hipStream_t st);
// everything else; sn is read only when g.scale is 0 (automatic)
hipError_t launch_paths(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, const PageGeometry& g, const PathsOptions& o,
                        const float* sn, const PathsOut& out, hipStream_t st);
