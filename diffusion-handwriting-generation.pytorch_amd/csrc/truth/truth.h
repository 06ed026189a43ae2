// truth.h — launchers and workspace layout of the page ground truth (include/dhw.h: dhw_truth); shared by
// truth.hip and dhw_truth_api.cpp.  What needs no device (sizes, argument rules) is in truth_host.h.  The scan, the line
// header and the tile constants are the page compositor's (page/page.h): a label map has dhw_page's geometry.
#pragma once
#include <hip/hip_runtime.h>

#include "../page/page.h"
#include "truth_host.h"

static_assert(TRUTH_MAX_G <= TRUTH_THREADS, "one thread places one group");

// the workspace of a call, by value
struct TruthWorkspace {
  PageLineHeader* hdr;   // [N]
  float4* segs;          // [N][L] drawn segments relative to the line's box corner (xmin, ymax), as the page compositor's
  int32_t* ids;          // [N][L] the label of each of them
};
inline TruthWorkspace truth_workspace(void* ws, int N, int L) {
  char* p = (char*)ws;
  TruthWorkspace w;
  w.hdr = (PageLineHeader*)p;
  w.segs = (float4*)(p + (size_t)N * PAGE_HEADER_BYTES);
  w.ids = (int32_t*)(p + (size_t)N * PAGE_HEADER_BYTES + (size_t)N * (size_t)L * PAGE_SEGMENT_BYTES);
  return w;
}

// the scan, every group's span and box, the line header; the labelled segments when want_segs.  With g.scale > 0 the boxes
// are placed and scale_out written; else they stay in stroke units (gxmin, gymax, gxmax, gymin) for launch_truth_place.
hipError_t launch_truth_prepare(const float* strokes, const int32_t* lens, const int32_t* slots, const int32_t* groups, int N, int L, int G,
                                const PageGeometry& g, bool want_segs, const TruthWorkspace& w, float* boxes_out, int32_t* spans_out,
                                float* scale_out, hipStream_t st);
// automatic scale only: s = min s_n, scale_out, and the boxes placed where they stand
hipError_t launch_truth_place(int N, int G, const PageGeometry& g, const TruthWorkspace& w, float* boxes_out, const int32_t* spans_out,
                              float* scale_out, hipStream_t st);
// the label map
hipError_t launch_truth_labels(int N, int L, const PageGeometry& g, const TruthWorkspace& w, int32_t* labels_out, hipStream_t st);
