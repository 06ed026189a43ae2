// sampler/handle.h — what the sampler's host units share: the handle, its workspaces and packed-weight records, the
// ConvBlock / tap ids, the error helpers, and the functions one unit offers the others.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../../include/dhw.h"
#include "../../../include/dhw_debug.h"
#include "../abi_guard.h"
#include "../dhw_kernels.h"
#include "../persist.h"
#include "plane_tag.h"
#include "../host/device_arena.h"
#include "../host/weight_store.h"

#pragma GCC visibility push(hidden)   // nothing below is exported: the library's dynamic symbols are the extern "C" entry points

constexpr int SIG = 32, SIG_HID = 2048, VOCAB = 73, STYLE_CH = 256;
constexpr int SLACK_ROWS = 64;   // every activation buffer is over-allocated so tile over-reads stay in bounds

struct ProfRec { int label; hipEvent_t a, b; double flops, bytes; int plane_call = -1; };   // plane_call: slot of h_prof_skip that says whether this launch was skipped
struct ProfAgg { std::string label; double ms = 0, flops = 0, bytes = 0; int64_t n = 0; };

struct Tap { void* p; int rows; int cols; bool f32; };
// dhw_debug_read's view of the last call: one slot per named activation, names resolved ONCE at dhw_create (build_names);
// a launch only touches slot ids.  (Round 4 kept a std::map<std::string, Tap> filled with names concatenated at every launch.)
struct TapSlot { std::string name; Tap t{}; bool set = false; };

// ConvBlocks and EncoderLayers by index: nothing on the launch path is looked up by name.
enum { CB_ENC1, CB_ENC2, CB_ENC4, CB_DEC3, CB_DEC2, CB_DEC1, CB_N };
constexpr const char* kConvName[CB_N] = {"enc1", "enc2", "enc4", "dec3", "dec2", "dec1"};
// EncoderLayer li: 0 = enc3, 1 = enc5, 2 + i = att_layers.i
enum { TAP_SIGMA_FFN, TAP_INPUT_DENSE, TAP_TS, TAP_TS_STYLE, TAP_TS_T2, TAP_ATT_DENSE, TAP_UP3, TAP_UP2, TAP_UP1,
       TAP_POOL1, TAP_POOL3, TAP_POOL5,   // AvgPool1d side outputs of enc1 / enc3 / enc5: the exact inputs of enc2 / enc4 / att_dense
       TAP_CONV0 };
inline int tap_conv(int id) { return TAP_CONV0 + id; }
constexpr int TAPS_PER_EL = 5;
inline int tap_el(int li, int which) { return TAP_CONV0 + CB_N + TAPS_PER_EL * li + which; }   // which: 0 = layer output, 1 = .x2, 2 = .x3, 3 = .k1, 4 = .v1

// One full activation workspace.  dhw_sample splits a prompt batch into independent sub-batches, each
// with its own workspace on its own (captured) stream, so several small kernels are in flight at once.
// Every buffer is a NAMED POINTER set by alloc_workspace / ensure_plane (dhw_create, or the first dhw_sample of a longer
// schedule): a buffer the launch sequence needs and the allocation code forgot is reported by need() as DHW_ERR_INTERNAL
// before anything is launched.  (Round 4: a std::map<std::string, void*> looked up with .at(name + ".k1") at every launch;
// a renamed buffer threw std::out_of_range through dhw_forward and aborted the host process.)
struct ConvBufs { void *h1 = nullptr, *h2 = nullptr, *out = nullptr; };
struct TextBufs { void *s1 = nullptr, *k8 = nullptr, *vt8 = nullptr, *t1 = nullptr, *q8 = nullptr, *a8 = nullptr, *t2 = nullptr, *tf_h = nullptr, *text_out = nullptr; };
struct EncTextBufs { void *tl = nullptr, *k1 = nullptr, *vt1 = nullptr; };
struct EncBufs {
  EncTextBufs t, tT;   // the layer's text-side projections: per call, and the all-steps plane
  void *q1 = nullptr, *a1 = nullptr, *x2 = nullptr, *qk2 = nullptr, *vt2 = nullptr, *a2 = nullptr, *x3 = nullptr, *f = nullptr, *out = nullptr;
};
struct Workspace {
  void *sty_in = nullptr, *sty_h = nullptr, *sty_n = nullptr, *t_n = nullptr;
  TextBufs ts, tsT;    // sigma-dependent text side: per call, and the all-steps plane (".T")
  void *x0 = nullptr, *enc1_pool = nullptr, *enc3_pool = nullptr, *enc5_pool = nullptr, *att_dense = nullptr;
  void* xd[3] = {nullptr, nullptr, nullptr};   // decoder inputs xd3, xd2, xd1 (DHW_FUSE_UP=0 only)
  ConvBufs cb[CB_N];
  std::vector<EncBufs> el;
  float* d_xt = nullptr;   // fp32 sampler state [B*L, 2]
  long cap_B = 0;          // prompts this workspace was sized for
  long plane_cap = 0;      // (steps x prompts) the all-steps text plane (".T" buffers) is sized for
  // what the last enqueued dhw_sample* call left in the ".T" buffers (dhw_debug_read_plane): the pair slots its chunking wrote,
  // the row count of a slot, and the plane allocation (plane_gen) the call's launches - or the graph it replayed - wrote into
  long plane_pairs = 0;
  int plane_Lt = 0;
  uint64_t plane_last_gen = 0;
};
constexpr int MAX_STREAMS = 8;

// one ConvBlock / EncoderLayer worth of packed weights
struct ConvBlockW {
  void *w_c1, *w_c2, *w_fc, *w_skip;
  float *b_c1, *b_c2, *b_fc, *b_skip;
  int cin, cout, f1, f2, f3;   // FiLM offsets
};
struct EncLayerW {
  void *w_td, *w_kv1, *w_q1, *w_d1, *w_qkv2, *w_d2, *w_f1, *w_f2;
  float *b_td, *b_kv1, *b_q1, *b_d1, *b_qkv2, *b_d2, *b_f1, *b_f2;
  float *pb_k1, *pb_q1, *pb_qk2;   // PE·W tables
  int d, heads, f0, f1, f2, f3;
  float pos_factor;
};

struct dhw_handle {
  dhw_dims dims{};      // PHYSICAL dims: what the kernels, workspaces and packed weights are sized for (c2 = 192)
  dhw_dims ldims{};     // the caller's dims (the reference's constructor arguments): c2 may be any multiple of 12 up to 192
  bool padded = false;  // ldims.c2 < dims.c2: weights are embedded into the physical shapes with zero padding (pad_weights)
  std::vector<KeySpec> pspec;                  // physical shapes, same key order as spec
  std::vector<std::vector<float>> phys_w;      // padded copies of store.host_w (padded handles only)
  int device = 0;
  int prec = 0;
  size_t es = 2;
  ErrBuf err;
  WeightStore store;    // the caller's state_dict: logical shapes (store.lookup_fail: a weight / FiLM name the packing code asked for does not exist)
  bool packed = false;
  DeviceArena arena;    // every device allocation of the handle, freed by destroy_impl

  // FiLM
  std::map<std::string, int> film_off;
  int film_tot = 0;
  float *d_film_w = nullptr, *d_film_b = nullptr;
  float *d_sig32 = nullptr, *d_film = nullptr, *d_sigma_in = nullptr;
  // dhw_sample: one FiLM table [T, 2*film_tot] per schedule length T, allocated once and never moved, so a cached graph
  // for T keeps reading ITS table whatever other T values are sampled in between (a single shared, re-grown buffer let a
  // replayed graph read another schedule's table).  d_film_T = the table of the call being enqueued.
  struct FilmT {
    float *d_sigma = nullptr, *d_sig32 = nullptr, *d_film = nullptr;
    std::vector<float> h_sigma;   // source of the async upload: must outlive the call
    bool ready = false;           // table computed for the current weights
  };
  std::map<int, FilmT> film_T;
  float* d_film_T = nullptr;

  // small fp32 weights
  float *sg_w1, *sg_b1, *sg_w2, *sg_b2, *in_w, *in_b, *out_w, *out_b, *pen_w, *pen_b, *emb;

  ConvBlockW enc1, enc2, enc4, dec3, dec2, dec1;
  std::vector<EncLayerW> el;   // enc3, enc5, att_layers...
  void *w_sf1, *w_sf3, *w_q8, *w_kv8, *w_d8, *w_tf1, *w_tf3, *w_attd, *w_sk1, *w_sk2, *w_sk3;
  float *b_sf1, *b_sf3, *b_q8, *b_kv8, *b_d8, *b_tf1, *b_tf3, *b_attd, *b_sk1, *b_sk2, *b_sk3;
  int f_ts1, f_ts2, f_ts3, f_ts4;

  // workspaces (ws[0] serves dhw_forward; dhw_sample uses ws[0..nstreams))
  std::vector<Workspace> ws;
  // sub-batches dhw_sample forks onto side streams (<= nstreams_alloc).  Default 1: on ROCm 7.2 parallel
  // hipGraph branches replay serially, and the split only shrinks every launch (measured 65 -> 99 ms at 4).
  int nstreams = 1;
  int nstreams_alloc = 1;
  hipStream_t sub_streams[MAX_STREAMS] = {};
  std::vector<TapSlot> taps;            // indexed by tap id (TAP_*, tap_conv, tap_el)
  std::vector<std::string> el_name;     // "enc3", "enc5", "att_layers.i"
  int lpadT = 0, lpadS = 0, lpadX[3] = {0, 0, 0};

  // profiling
  bool prof = false;
  std::vector<std::string> prof_labels;
  std::vector<ProfRec> prof_recs;
  std::vector<ProfAgg> prof_agg;

  // graph cache for dhw_sample: the graph only touches library-owned staging buffers, so it is keyed by the
  // problem shape alone and replays for any caller pointers
  bool use_graph = true;
  // teacher forcing of dhw_sample (dhw_debug_set_teacher): every `teach_every` steps x is captured and replaced
  int teach_every = 0;
  const float* teach_reset = nullptr;
  float* teach_capture = nullptr;
  bool fuse_heads = true;       // dec1 evaluates heads + scheduler step (env DHW_FUSE_HEADS=0 -> separate launch)
  bool plane = true;            // all-steps text plane in dhw_sample (env DHW_PLANE=0 -> text side inside every step)
  bool fuse_up = true;          // decoder ConvBlocks evaluate Upsample + skip_conv while staging (env DHW_FUSE_UP=0 -> separate GEMM)
  bool chain = true;            // row-local stages continue across layer boundaries inside one launch (env DHW_CHAIN=0 -> off)
  bool fuse = true;             // fused block kernels (env DHW_FUSE=0 -> one launch per GEMM, for A/B runs)
  bool fuse_text = true;        // fused text-side kernels (textside.hip; env DHW_FUSE_TEXT=0 -> generic GEMM / attention launches)
  // how the stroke kernels' tile copy-outs store (dhw_kernels.h STORE_*): two bits per output class, C | A << 2 | B << 4
  // (env DHW_STORE_POLICY, read once at dhw_create; part of the graph / plan key like the switches above).  The default word is
  // compiled into convblock.hip / enclayer.hip; any other runs the *_policy launchers, which read it from the parameter blocks.
  int store_policy = DHW_STORE_DEFAULT;
  int text_pairs = 0;           // (step, prompt) pairs per workgroup of text_layer_kernel: 0 = by size, env DHW_TEXT_PAIRS = 1 / 2 forces one form
  std::map<std::vector<uint64_t>, hipGraphExec_t> graphs;
  std::map<std::vector<uint64_t>, uint64_t> graph_plane_gen;   // per cached graph: plane_gen when it was captured (it keeps those ".T" buffers)
  int64_t* d_text_stage = nullptr;
  float* d_style_stage = nullptr;
  float* d_out_stage = nullptr;
  float* d_noise_stage = nullptr;
  size_t noise_stage_cap = 0;
  // conditioned calls (dhw_sample_cond): known [max_B*max_L, 3] and keep [max_B*max_L] are allocated once, at the first such
  // call, and never move; the conditioning noise [T, B, L, 2] grows like the noise stage (cached graphs and plans dropped first)
  float* d_known_stage = nullptr;
  unsigned char* d_keep_stage = nullptr;
  float* d_cond_noise_stage = nullptr;
  size_t cond_noise_stage_cap = 0;
  // the eager entries around the denoiser (dhw_score, dhw_ddim_sample, dhw_ddim_invert): x, w, eps [max_B*max_L, 2], pen
  // [max_B*max_L] and sigma [max_B], allocated once, at the first such call (ensure_scratch), and never moved.  dhw_score keeps
  // x_t in x and its draw z in w; the ddim entries keep the state in x and the inversion's iterate in w; eps, pen and sigma are
  // the denoiser's outputs and input for both.  The entries share the set as they share ws[0]: all of them launch eagerly on
  // the caller's stream, and within a call every row p < lens[b] is written before a launch of that call reads it, while rows
  // at or past lens[b] are never read.  No graph reads the set: these calls leave the cached graphs alone.  hist [max_B*max_L, 2]
  // is the set's fifth buffer: the previous step's x0 estimate of dhw_dpm_sample / dhw_guided_dpm_sample, allocated at the first
  // such call (step/dhw_step_api.cpp) and never moved; step 0 of a call writes it before any step reads it.
  struct DenoiseScratch { float *x = nullptr, *w = nullptr, *eps = nullptr, *pen = nullptr, *sigma = nullptr, *hist = nullptr; } scratch;
  uint64_t* d_seed = nullptr;   // [seed, first_sample] read by the noise kernels
  // Reuse of the all-steps text plane across dhw_sample* calls.  plane_tag: what the plane in the ".T" buffers was
  // computed for; cleared by everything that may change it (plane_invalidate) and while a call is being enqueued.
  // d_plane_skip[0]: 1 = the plane is valid for the call in flight (set_seed_kernel writes the host's verdict, stage_compare_kernel
  // clears it when prompts or styles differ, text_style_kernel / text_layer_kernel read it inside the graph); [1]: earlier calls that reused.
  bool plane_reuse = true;      // env DHW_PLANE_REUSE=0 -> the host's verdict is always 0
  PlaneTag plane_tag;
  uint64_t weights_gen = 0, plane_gen = 0;
  unsigned* d_plane_skip = nullptr;
  long plane_calls = 0;         // dhw_sample* calls enqueued on this handle
  // profile mode: the flag of every call, copied behind its compare into a pinned slot, so that the rows of skipped launches
  // can report no work once the events are resolved
  unsigned* h_prof_skip = nullptr;
  int prof_calls = 0;
  static constexpr int PROF_SKIP_CAP = 4096;
  // ragged calls (dhw_forward_ragged / dhw_sample_ragged): the per-sample lengths, copied on the caller's stream from a pinned host
  // buffer the handle owns.  The kernels read them at run time, so one captured graph serves every set of lengths of a shape.
  int* d_lens = nullptr;          // [max_B]
  int* h_lens_pin = nullptr;      // [max_B] pinned source of that copy
  hipEvent_t lens_ev = nullptr;   // recorded behind the last copy: the pinned buffer is rewritten only once that copy has read it
  // guided calls (dhw_guided_ddim_sample / dhw_guided_sample, step/dhw_step_api.cpp): the per-sample scales, staged like the lengths.
  // Allocated at the first guided call (the device array in the arena) and never moved.
  float* d_guide_scale = nullptr;       // [max_B]
  float* h_guide_scale_pin = nullptr;   // [max_B] pinned source of that copy
  hipEvent_t guide_ev = nullptr;        // recorded behind the last copy

  // One persistent launch per denoiser call inside dhw_sample's graph (persist.h): env DHW_PERSIST=1.  OFF by default: measured
  // 359 us per call against 328 us for the eleven launches (profiles/r04_persistent_step_trace.log) — bit-identical
  // samples, but every hand-off costs what a kernel boundary costs and the merged kernel's bodies compile worse.  One StepPlan
  // per sampler step, built by running the launch sequence in record mode, keyed like the graphs.
  bool persist = false;
  int persist_grid = 0;               // resident workgroups to start = the device's CU count
  unsigned* d_step_sync = nullptr;    // tickets / per-sample counters (zero between launches)
  size_t step_sync_words = 0;
  unsigned* h_step_err = nullptr;     // host-mapped error word of the step kernels (bounded spins), and its device address
  unsigned* d_step_err = nullptr;
  struct StepPlans { StepPlan* dev = nullptr; bool ok = false; };
  unsigned long long* d_step_trace = nullptr;   // diagnostics (DHW_PERSIST_TRACE=1): [workgroup][phase][4] stamps of the LAST step of a call
  std::map<std::vector<uint64_t>, StepPlans> plans;

  int last_B = 0, last_L = 0, last_Lt = 0;
};

int fail(dhw_handle* h, int code, const char* fmt, ...) noexcept;   // (dhw_api.cpp) records the message, returns code

// the layer's text values are kept as rows [B*Lt, d] (fused bf16 EncoderLayer kernels) instead of transposed [B][d][lpadT]
inline bool v_rows(const dhw_handle* h, const EncLayerW& w) { return h->fuse && h->prec == PREC_BF16 && enclayer_supported(h->prec, w.d, w.heads); }

// The conditioning block of dhw_sample_cond (include/dhw.h), as the caller passed it: device pointers or null.
struct CondArgs {
  const float* known;
  const uint8_t* keep;
  int t_start;
  const float* cond_noise;
};

// The body of every extern "C" entry point runs inside this: no exception leaves the library (abi_guard.h).
#define DHW_GUARD(h, fn, R, ...) \
  return abi_guard<R>(fn, [&](const char* f_, const char* w_) { return fail((h), DHW_ERR_INTERNAL, "%s: internal error: %s", f_, w_); }, [&]() -> R __VA_ARGS__)

#define HIPCK(h, call)                                                                                  \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return fail(h, DHW_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// a DeviceArena call of the handle: the message names the HIP call that failed, as HIPCK does
#define ARENACK(h, call)                                                                                 \
  do {                                                                                                   \
    hipError_t e_ = (h)->arena.call;                                                                     \
    if (e_ != hipSuccess) return fail(h, DHW_ERR_HIP, "%s failed: %s (%s:%d)", (h)->arena.failed, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// ---------------------------------------------------------------- sampler/weights.cpp
std::vector<KeySpec> build_spec(int nl, int c1, int c2, int c3);
void build_film_layout(dhw_handle* h);
int true_width(const dhw_handle* h, int n);
int finalize_impl(dhw_handle* h);

// ---------------------------------------------------------------- sampler/workspace.cpp
int dev_alloc(dhw_handle* h, void** p, size_t bytes, bool zero = true);
long el_rows(long L, int li);
int alloc_workspace(dhw_handle* h, Workspace& w, long B);
int ensure_plane(dhw_handle* h, Workspace& w, long steps, long B);
int alloc_shared(dhw_handle* h);
int verify_workspace(dhw_handle* h, const Workspace& w);
void build_names(dhw_handle* h);
void destroy_impl(dhw_handle* h);
void drop_graphs(dhw_handle* h);     // destroy every cached graph of dhw_sample (the caller has synchronised the device)
int ensure_scratch(dhw_handle* h);   // h->scratch, at the handle's capacity, at the first call that needs it

// ---------------------------------------------------------------- sampler/sample.cpp
void schedule_host(int T, std::vector<float>& beta, std::vector<float>& alpha);
std::vector<float> schedule_abar(int T);   // alpha alone: what the level tables of dhw_score and the ddim entries index
int check_shapes(dhw_handle* h, int B, int L, int Lt, const char* fn = nullptr);   // fn: the message opens with "<fn>: "
int check_lens(dhw_handle* h, const char* fn, const int32_t* lens, int B, int L, bool sampling);
int stage_lens(dhw_handle* h, const int32_t* lens, int B, hipStream_t st);   // the copy of checked lengths to h->d_lens
int forward_enqueue(dhw_handle* h, const float* strokes, const int64_t* text, const float* sigma, const float* style, int B, int L, int Lt,
                    float* eps_out, float* pen_out, hipStream_t st, const int* lens);
int forward_impl(dhw_handle* h, const char* fn, const float* strokes, const int64_t* text, const float* sigma, const float* style,
                 int B, int L, int Lt, float* eps_out, float* pen_out, void* hip_stream, const int32_t* lens_host, bool ragged);
int sample_impl(dhw_handle* h, const char* fn, const int64_t* text, const float* style, int B, int L, int Lt, int T, int mode,
                const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream, const int32_t* lens_host, bool ragged,
                const CondArgs* cond = nullptr);
int work_impl(dhw_handle* h, int L, int Lt, double* flops_out, double* bytes_out);

// ---------------------------------------------------------------- sampler/debug.cpp
int64_t debug_read(dhw_handle* h, const char* name, float* host_dst, int64_t max_floats, int64_t shape_out[3]);
int64_t debug_read_plane(dhw_handle* h, int workspace_slot, const char* name, float* host_dst, int64_t max_floats, int64_t shape_out[3]);
int debug_raise(dhw_handle* h, int kind);
int debug_randn(dhw_handle* h, uint64_t seed, int64_t first_sample, int B, int L, int iter, float* host_dst);
int debug_attention_time(dhw_handle* h, int layer, int iters, double* us_with, double* us_without, double* flops_out, void* hip_stream);
int profile_enable(dhw_handle* h, int on);
int profile_reset(dhw_handle* h);
int profile_count(dhw_handle* h);
int profile_get(dhw_handle* h, int i, const char** label, double* total_ms, int64_t* launches, double* flops_sum, double* bytes_sum);
int set_streams(dhw_handle* h, int n);
int debug_persist_plans(dhw_handle* h);
int debug_persist_trace(dhw_handle* h, unsigned long long* host_dst, int64_t max_words);
int set_graph(dhw_handle* h, int on);
int debug_plane_reuse(dhw_handle* h, int* last, long* calls, long* reused);
inline void plane_invalidate(dhw_handle* h) { h->plane_tag.valid = false; }   // the resident plane is no longer known to match anything
int debug_set_teacher(dhw_handle* h, const float* reset_dev, float* capture_dev, int every);

#pragma GCC visibility pop
