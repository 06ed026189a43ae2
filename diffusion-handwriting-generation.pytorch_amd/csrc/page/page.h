// page.h — launchers and workspace layout of the page compositor (include/dhw.h: dhw_page); shared by
// page.hip and dhw_page_api.cpp.  What needs no device (sizes, argument rules) is in page_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "page_host.h"

constexpr int PAGE_ITEMS = PAGE_MAX_L / PAGE_THREADS;   // strokes per thread of the prepare kernel (fixed, so the summation
                                                        // order depends on the stroke index alone)
constexpr int PAGE_CHUNK = 256;                         // segments per LDS chunk of the raster kernel

// What the prepare kernel leaves per line.  count = 0: the line draws nothing (no drawn segment, or its slot is off the
// pages) and takes no part in the scale; its s_n is +inf.
struct PageLineHeader {
  int32_t count;          // drawn segments
  float xmin, ymax;       // the corner of the ink box the segments are relative to
  float ex, ey;           // the extents of the ink box, stroke units
  float s_n;              // the largest scale at which this line fits its slot (+inf: no constraint)
  int32_t slot;
  int32_t pad;
};
static_assert(sizeof(PageLineHeader) == PAGE_HEADER_BYTES, "page_host.h sizes the workspace");
static_assert(sizeof(float4) == PAGE_SEGMENT_BYTES, "page_host.h sizes the workspace");

hipError_t launch_page_prepare(const float* strokes, const int32_t* lens, const int32_t* slots, int N, int L, const PageGeometry& g,
                               PageLineHeader* hdr, float4* segs, hipStream_t st);
hipError_t launch_page_raster(const PageLineHeader* hdr, const float4* segs, int N, int L, const PageGeometry& g, float* pages,
                              float* scale_out, float* boxes_out, hipStream_t st);
