// prep.h — launcher of the writer-image preparation (include/dhw.h: dhw_prep); shared by prep.hip and dhw_prep_api.cpp.
// Definition of the result: include/dhw.h and DESIGN.md §26.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prep_host.h"

constexpr int PREP_THREADS = 256;
constexpr int PREP_BOX_COLS = 64 * 16;   // box pass: a workgroup covers 64 lanes x 16 bytes of every row of its strip
constexpr int PREP_BOX_ROWS = 64;        //           and a strip of this many rows, 16 per wave
constexpr int PREP_TILE_COLS = 64 * 4;   // resize pass: a workgroup covers 64 threads x 4 output columns
constexpr int PREP_BAND_ROWS = 32;       //              and a band of this many output rows, 8 per wave

// init, box pass, resize pass on one stream; `boxes` is the workspace, int32 [B][4]
hipError_t launch_prep(const uint8_t* images, const int32_t* sizes, int B, int Hin, int Win, int H, int W, int thresh, float* img_out,
                       int32_t* widths_out, int32_t* boxes_out, int32_t* status_out, int32_t* boxes, hipStream_t st);
