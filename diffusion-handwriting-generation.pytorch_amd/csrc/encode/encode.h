// encode.h — launcher of the stroke encoder (include/dhw.h: dhw_encode); shared by encode.hip and dhw_encode_api.cpp.
// Definition of the result: include/dhw.h and DESIGN.md §25.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "encode_host.h"

constexpr int ENCODE_THREADS = 256;
constexpr int ENCODE_SMALL_N = 1024;   // lines of at most this many points run in the 21 KiB instance of the kernel (several
                                       // workgroups per CU), longer ones in the 84 KiB one; both do the same arithmetic

hipError_t launch_encode(const float* points, const int32_t* counts, int B, int N, int L, int rounds, float max_abs,
                         float* strokes_out, int32_t* lens_out, int32_t* status_out, hipStream_t st);
