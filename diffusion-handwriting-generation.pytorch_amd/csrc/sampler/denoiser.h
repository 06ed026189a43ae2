// sampler/denoiser.h — the launch context of the denoiser (sampler/denoiser.cpp) as the sampling loop and the debug hooks
// see it: Ctx, the checked workspace accessors, the per-launch profiling bracket.
#pragma once
#include "handle.h"

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------- profiling wrapper
struct Launch {
  dhw_handle* h;
  hipStream_t st;
  int rec = -1;
  // plane_call: >= 0 for a launch that the plane-reuse flag of that profiled call may have skipped (handle.h h_prof_skip)
  Launch(dhw_handle* h_, hipStream_t st_, const char* label, double flops = 0, double bytes = 0, int plane_call = -1) : h(h_), st(st_) {
    if (!h->prof) return;
    int id = -1;
    for (size_t i = 0; i < h->prof_labels.size(); ++i)
      if (h->prof_labels[i] == label) id = (int)i;
    if (id < 0) { id = (int)h->prof_labels.size(); h->prof_labels.push_back(label); }
    ProfRec r{id, nullptr, nullptr, flops, bytes, plane_call};
    hipEventCreate(&r.a);
    hipEventCreate(&r.b);
    hipEventRecord(r.a, st);
    h->prof_recs.push_back(r);
    rec = (int)h->prof_recs.size() - 1;
  }
  ~Launch() {
    if (rec >= 0) hipEventRecord(h->prof_recs[rec].b, st);
  }
};

// ---------------------------------------------------------------- the denoiser launch sequence
struct Ctx {
  dhw_handle* h;
  Workspace* ws;
  hipStream_t st;
  int B, L, Lt, S5;
  const float* film;   // row 0 of the FiLM table to use
  long film_bs;        // FiLM row stride (0 in the sampling loop)
  int err = 0;
  int film_div = 1;    // samples per FiLM row
  int in_B = 0;        // batch of the sigma-independent inputs (0 = B); the text plane replicates them over steps
  bool planeT = false; // the text side writes the all-steps plane (".T" buffers) instead of the per-call ones
  const unsigned* plane_skip = nullptr;   // planeT only: the fused text-side launches return at once when *plane_skip != 0
  int plane_call = -1;      // profile mode: this call's slot of h_prof_skip
  const HeadsParams* fhp = nullptr;   // sampling loop: dec1 evaluates the heads + scheduler step itself
  bool fuse_input = false;  // enc1 evaluates input_dense while staging (sampling loop); forward() keeps the tap
  bool use_plane = false;   // stroke path reads the text K/V of step `plane_step` from the plane
  long plane_step = 0;
  // record mode (persist.h): the fused launches of stroke_path are appended to `rec` as phases instead of being launched;
  // anything the persistent kernel has no phase for sets rec_fail
  std::vector<StepPhase>* rec = nullptr;
  bool rec_fail = false;
  const int* lens = nullptr;   // ragged batch: device lengths of samples [0, B) at full resolution (GemmParams.lens), or null
};

// A workspace pointer the launch sequence is about to hand to a kernel.  All of them are set when the workspace is allocated
// (alloc_workspace at dhw_create, ensure_plane); one that is still null here is a bug in that code: it becomes a status
// (every launch helper checks c.err first) — not a throw across the ABI and not a null dereference on the device.
void* need(Ctx& c, void* p, const char* what);
#define WS(c, field) need((c), (c).ws->field, #field)
#define TS(c, field) need((c), ((c).planeT ? (c).ws->tsT : (c).ws->ts).field, (c).planeT ? #field ".T" : #field)          /* sigma-dependent text side */
#define CBB(c, id, field) need((c), (c).ws->cb[id].field, #field)                                                        /* ConvBlock id */
#define ELB(c, li, field) need((c), (c).ws->el[li].field, #field)                                                        /* EncoderLayer li */
#define ELT(c, li, field) need((c), ((c).planeT ? (c).ws->el[li].tT : (c).ws->el[li].t).field, (c).planeT ? #field ".T" : #field)   /* its text projections, as the text side writes them */
#define ELK(c, li, field) need((c), ((c).use_plane ? (c).ws->el[li].tT : (c).ws->el[li].t).field, (c).use_plane ? #field ".T" : #field)   /* ... as the stroke side reads them */

#define RUN_SMALL(c, label, call)                                                                  \
  do {                                                                                             \
    if ((c).rec) (c).rec_fail = true;                                                              \
    else if (!(c).err) {                                                                                \
      Launch l_((c).h, (c).st, label);                                                             \
      hipError_t e_ = (call);                                                                      \
      if (e_ != hipSuccess) (c).err = fail((c).h, DHW_ERR_HIP, "%s: %s", label, hipGetErrorString(e_)); \
    }                                                                                              \
  } while (0)

void run_gemm(Ctx& c, const char* label, const GemmParams& p);   // one generic GEMM launch (p.lens: the ragged launcher), profiled under `label`
void tap(Ctx& c, int id, void* p, int rows, int cols, bool f32 = false);
void taps_clear(dhw_handle* h);
EncLayerParams enc_params(Ctx& c, int li, const EncLayerW& w, const void* x, int Lk, int lpad, const int64_t* text, void* pool);
void text_style_static(Ctx& c, const int64_t* text, const float* style);
void text_style_dynamic(Ctx& c);
void stroke_path(Ctx& c, const float* strokes, const int64_t* text);
int launch_heads_for(Ctx& c, HeadsParams hp);

// ---------------------------------------------------------------- the eager entries (sampler/sample.cpp)
// dhw_forward*, dhw_score, dhw_ddim_sample / _invert and dhw_attention open alike: the entry's own null-pointer line,
// eager_check (no HIP call: the limits of B, L, Lt, under the entry's name when name_shapes is set, and of lens when given),
// the entry's own checks, eager_begin (dhw_finalize, the device, the copy of lens to h->d_lens on the stream), the work.
struct EagerCall {
  hipStream_t st;
  const int* lens;   // h->d_lens of a ragged call, or null
  Ctx small;         // for the entry's own small launches (RUN_SMALL): ws[0], FiLM row stride 0
};
int eager_check(dhw_handle* h, const char* fn, int B, int L, int Lt, const int32_t* lens, bool name_shapes = false);
int eager_begin(dhw_handle* h, int B, int L, int Lt, const int32_t* lens, void* hip_stream, EagerCall* ec);

#pragma GCC visibility pop
