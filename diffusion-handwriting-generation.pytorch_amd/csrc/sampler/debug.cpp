// sampler/debug.cpp — the debug / measurement hooks of include/dhw_debug.h and the profiling, stream and graph switches.
#include <algorithm>
#include <new>

#include "denoiser.h"

// ---------------------------------------------------------------- debug / measurement hooks
int64_t debug_read(dhw_handle* h, const char* name, float* host_dst, int64_t max_floats, int64_t shape_out[3]) {
  if (!h || !name || !host_dst) return fail(h, DHW_ERR_ARG, "dhw_debug_read: null argument");
  const Tap* tp = nullptr;
  for (const TapSlot& sl : h->taps)
    if (sl.set && sl.name == name) tp = &sl.t;
  if (!tp) return fail(h, DHW_ERR_ARG, "no activation named %s", name);
  const Tap& t = *tp;
  const int64_t n = (int64_t)h->last_B * t.rows * t.cols;
  if (n > max_floats) return fail(h, DHW_ERR_ARG, "buffer too small for %s", name);
  if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(h, DHW_ERR_HIP, "sync failed: %s", hipGetErrorString(hipGetLastError()));
  if (shape_out) { shape_out[0] = h->last_B; shape_out[1] = t.rows; shape_out[2] = t.cols; }
  if (t.f32 || h->prec == PREC_F32) {
    if (hipMemcpy(host_dst, t.p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DHW_ERR_HIP, "memcpy failed");
  } else {
    std::vector<uint16_t> tmp(n);
    if (hipMemcpy(tmp.data(), t.p, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DHW_ERR_HIP, "memcpy failed");
    for (int64_t i = 0; i < n; ++i) host_dst[i] = bf2f(tmp[i]);
  }
  return n;
}

// The all-steps text plane of workspace `slot` as the last dhw_sample* call left it: "text_style_model" [pairs, Lt, 2 c2],
// "<layer>.k1" [pairs, Lt, d], "<layer>.v1" as stored ([pairs, Lt, d] rows, or V^T [pairs, d, lpadT]).  pairs = every slot the
// call's chunking wrote (Workspace::plane_pairs).  Reads only: the plane tag and the reuse flag are left alone.
int64_t debug_read_plane(dhw_handle* h, int slot, const char* name, float* host_dst, int64_t max_floats, int64_t shape_out[3]) {
  if (!h || !name || !host_dst) return fail(h, DHW_ERR_ARG, "dhw_debug_read_plane: null argument");
  if (slot < 0 || slot >= (int)h->ws.size()) return fail(h, DHW_ERR_ARG, "dhw_debug_read_plane: no workspace %d", slot);
  const Workspace& w = h->ws[slot];
  if (!h->plane || !w.plane_cap) return fail(h, DHW_ERR_STATE, "dhw_debug_read_plane: the handle has no all-steps text plane");
  if (!w.plane_pairs) return fail(h, DHW_ERR_STATE, "dhw_debug_read_plane: no dhw_sample call has written the plane of workspace %d", slot);
  if (w.plane_last_gen != h->plane_gen || w.plane_pairs > w.plane_cap)
    return fail(h, DHW_ERR_STATE, "dhw_debug_read_plane: the last call replayed a graph that writes an earlier allocation of the plane");
  const std::string nm(name);
  const void* src = nullptr;
  int64_t rows = w.plane_Lt, cols = 0;
  if (nm == "text_style_model") {
    src = w.tsT.text_out;
    cols = 2 * h->dims.c2;
  } else {
    for (size_t li = 0; li < h->el.size() && li < w.el.size() && !src; ++li) {
      const EncLayerW& lw = h->el[li];
      if (nm == h->el_name[li] + ".k1") {
        src = w.el[li].tT.k1;
        cols = lw.d;
      } else if (nm == h->el_name[li] + ".v1") {
        src = w.el[li].tT.vt1;
        if (v_rows(h, lw)) cols = lw.d;
        else { rows = lw.d; cols = h->lpadT; }
      }
    }
  }
  if (!src) return fail(h, DHW_ERR_ARG, "no plane buffer named %s", name);
  const int64_t n = w.plane_pairs * rows * cols;
  if (n > max_floats) return fail(h, DHW_ERR_ARG, "buffer too small for %s", name);
  if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(h, DHW_ERR_HIP, "sync failed: %s", hipGetErrorString(hipGetLastError()));
  if (shape_out) { shape_out[0] = w.plane_pairs; shape_out[1] = rows; shape_out[2] = cols; }
  if (h->prec == PREC_F32) {
    if (hipMemcpy(host_dst, src, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DHW_ERR_HIP, "memcpy failed");
  } else {
    std::vector<uint16_t> tmp(n);
    if (hipMemcpy(tmp.data(), src, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DHW_ERR_HIP, "memcpy failed");
    for (int64_t i = 0; i < n; ++i) host_dst[i] = bf2f(tmp[i]);
  }
  return n;
}

// Tests of the no-throw barrier itself (needs no device, handle may be null): raise a C++ exception INSIDE the guarded body of an
// entry point, exactly where a std::map::at / vector::resize / new of the host code would.  Must come back as DHW_ERR_INTERNAL.
int debug_raise(dhw_handle* h, int kind) {
  if (kind == DHW_RAISE_OUT_OF_RANGE) {
    std::map<std::string, int> m;
    return m.at("a buffer that was never allocated");
  }
  if (kind == DHW_RAISE_BAD_ALLOC) throw std::bad_alloc();
  if (kind == DHW_RAISE_UNKNOWN) throw 42;
  return fail(h, DHW_ERR_ARG, "dhw_debug_raise: kind %d", kind);
}

int debug_randn(dhw_handle* h, uint64_t seed, int64_t first_sample, int B, int L, int iter, float* host_dst) {
  if (!h || !host_dst || B < 1 || L < 1 || iter < -1 || (long)B * L > (long)h->dims.max_B * h->dims.max_L)
    return fail(h, DHW_ERR_ARG, "dhw_debug_randn: bad argument");
  HIPCK(h, hipSetDevice(h->device));
  HIPCK(h, hipDeviceSynchronize());
  const long rows = (long)B * L;
  hipError_t e = launch_set_seed(h->d_seed, seed, first_sample, nullptr);
  if (e == hipSuccess) e = launch_randn_init(h->ws[0].d_xt, rows, L, h->d_seed, 0, nullptr, iter);
  if (e != hipSuccess) return fail(h, DHW_ERR_HIP, "randn: %s", hipGetErrorString(e));
  HIPCK(h, hipMemcpy(host_dst, h->ws[0].d_xt, rows * 2 * 4, hipMemcpyDeviceToHost));
  return 0;
}

// The self-attention stage of an EncoderLayer's second kernel on its own (bench.py, roofline.by_function.attention; north_star:
// "MFMA utilisation for attention against the chip's peak").  enc_bc_kernel of layer `layer` (0 = enc3, 1 = enc5, 2.. = the
// bottleneck layers) is launched `iters` times back to back WITH its attention stage and `iters` times with the stage skipped
// (EncLayerParams.dbg bit 0, csrc/enc_bc_core.h) on the buffers the LAST dhw_forward(B, L, Lt) left in the workspace; the
// difference of the two mean launch times (HIP events on the stream) is the time of QK^T + softmax + PV + K / V staging.
// The product kernel, unmodified: no stamps, no extra instantiation.  flops_out = 4 B Lk^2 d (QK^T and PV over all heads).
int debug_attention_time(dhw_handle* h, int layer, int iters, double* us_with, double* us_without, double* flops_out, void* hip_stream) {
  if (!h || !us_with || !us_without || iters < 1 || layer < 0) return fail(h, DHW_ERR_ARG, "dhw_debug_attention_time: bad argument");
  if (!h->packed || !h->last_B || layer >= (int)h->el.size()) return fail(h, DHW_ERR_STATE, "dhw_debug_attention_time: run dhw_forward first (layer %d of %d)", layer, (int)h->el.size());
  const EncLayerW& w = h->el[layer];
  if (!h->fuse || h->prec != PREC_BF16 || !enclayer_supported(h->prec, w.d, w.heads)) return fail(h, DHW_ERR_STATE, "dhw_debug_attention_time: the fused bf16 EncoderLayer kernels are not in use on this handle");
  HIPCK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const int B = h->last_B, L = h->last_L;
  const int Lk = (int)el_rows(L, layer);
  Ctx c{h, &h->ws[0], st, B, L, h->last_Lt, h->dims.S * 5, h->d_film, 2L * h->film_tot};
  const void* x = layer == 0 ? CBB(c, CB_ENC2, out) : layer == 1 ? CBB(c, CB_ENC4, out) : layer == 2 ? WS(c, att_dense) : ELB(c, layer - 1, out);
  EncLayerParams q = enc_params(c, layer, w, x, Lk, h->lpadX[layer < 2 ? layer : 2], h->d_text_stage, nullptr);   // (reads the stage; the plane tag stays)
  // (the measured launches write the layer's `out` again: same inputs, same values; with the stage skipped, different ones —
  // the workspace is scratch between calls)
  if (c.err) return c.err;
  hipEvent_t e0, e1;
  HIPCK(h, hipEventCreate(&e0));
  HIPCK(h, hipEventCreate(&e1));
  double us[2] = {0, 0};
  int rc = 0;
  for (int mode = 0; mode < 2 && !rc; ++mode) {
    q.dbg = mode;   // 0: with the attention stage, 1: skipped
    for (int it = 0; it < 3 + iters && !rc; ++it) {
      if (it == 3 && hipEventRecord(e0, st) != hipSuccess) rc = fail(h, DHW_ERR_HIP, "event record failed");
      hipError_t e = launch_enclayer(h->prec, q, 1, st, nullptr);
      if (e != hipSuccess) rc = fail(h, DHW_ERR_HIP, "enc_bc launch: %s", hipGetErrorString(e));
    }
    float ms = 0.f;
    if (!rc && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
      rc = fail(h, DHW_ERR_HIP, "event timing failed: %s", hipGetErrorString(hipGetLastError()));
    us[mode] = (double)ms * 1e3 / iters;
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (rc) return rc;
  *us_with = us[0];
  *us_without = us[1];
  if (flops_out) *flops_out = 4.0 * B * (double)Lk * Lk * w.d;
  return 0;
}

// (profiled calls launch eagerly into the same ".T" buffers and evaluate the same kernels: the resident plane stays valid)
int profile_enable(dhw_handle* h, int on) {
  if (!h) return DHW_ERR_ARG;
  if (on && !h->h_prof_skip && (hipSetDevice(h->device) != hipSuccess || hipHostMalloc((void**)&h->h_prof_skip, dhw_handle::PROF_SKIP_CAP * sizeof(unsigned)) != hipSuccess))
    return fail(h, DHW_ERR_HIP, "pinned plane-flag buffer: %s", hipGetErrorString(hipGetLastError()));
  h->prof = on != 0;
  return 0;
}
int profile_reset(dhw_handle* h) {
  if (!h) return DHW_ERR_ARG;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  for (auto& r : h->prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  h->prof_recs.clear();
  h->prof_agg.clear();
  h->prof_calls = 0;
  return 0;
}
int profile_count(dhw_handle* h) {
  if (!h) return DHW_ERR_ARG;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  h->prof_agg.assign(h->prof_labels.size(), ProfAgg{});
  for (size_t i = 0; i < h->prof_labels.size(); ++i) h->prof_agg[i].label = h->prof_labels[i];
  for (auto& r : h->prof_recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    ProfAgg& a = h->prof_agg[r.label];
    // a text-plane launch of a call that reused the resident plane returned at once: its time counts, its algorithmic work does not
    const bool skipped = r.plane_call >= 0 && h->h_prof_skip && h->h_prof_skip[r.plane_call] != 0;
    a.ms += ms; a.flops += skipped ? 0.0 : r.flops; a.bytes += skipped ? 0.0 : r.bytes; a.n += 1;
  }
  return (int)h->prof_agg.size();
}
int profile_get(dhw_handle* h, int i, const char** label, double* total_ms, int64_t* launches, double* flops_sum,
                    double* bytes_sum) {
  if (!h || i < 0 || i >= (int)h->prof_agg.size()) return DHW_ERR_ARG;
  const ProfAgg& a = h->prof_agg[i];
  if (label) *label = a.label.c_str();
  if (total_ms) *total_ms = a.ms;
  if (launches) *launches = a.n;
  if (flops_sum) *flops_sum = a.flops;
  if (bytes_sum) *bytes_sum = a.bytes;
  return 0;
}
int set_streams(dhw_handle* h, int n) {
  if (!h || n < 1) return DHW_ERR_ARG;
  h->nstreams = std::min(n, h->nstreams_alloc);
  plane_invalidate(h);   // (the sub-batch split decides which workspace's plane holds which prompts)
  return h->nstreams;
}
// shapes of dhw_sample that run as one persistent launch per denoiser call (persist.h): cached plans that are in use
int debug_persist_plans(dhw_handle* h) {
  if (!h) return DHW_ERR_ARG;
  int n = 0;
  for (auto& kv : h->plans) n += kv.second.ok ? 1 : 0;
  return n;
}
// diagnostics: the stamps of the last persistent step (see persist.hip, PTRACE) -> host_dst[workgroups * STEP_MAX_PHASES * 4]; returns
// the number of workgroups (0 = no trace buffer: DHW_PERSIST_TRACE was not set when the plans were built)
int debug_persist_trace(dhw_handle* h, unsigned long long* host_dst, int64_t max_words) {
  if (!h || !host_dst) return DHW_ERR_ARG;
  if (!h->d_step_trace) return 0;
  const int64_t n = (int64_t)h->persist_grid * STEP_MAX_PHASES * 4;
  if (max_words < n) return DHW_ERR_ARG;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_dst, h->d_step_trace, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return DHW_ERR_HIP;
  return h->persist_grid;
}
int set_graph(dhw_handle* h, int on) {
  if (!h) return DHW_ERR_ARG;
  h->use_graph = on != 0;
  plane_invalidate(h);   // every dhw_set_* clears the tag: the first call after a switch evaluates the text side
  return 0;
}

// The plane-reuse flag of the most recent dhw_sample* call, read back from the device, and the counts: calls enqueued, and how
// many of them ran with the flag set (the device folds each finished call's flag into a counter when the next one opens).
int debug_plane_reuse(dhw_handle* h, int* last, long* calls, long* reused) {
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  HIPCK(h, hipSetDevice(h->device));
  HIPCK(h, hipDeviceSynchronize());
  unsigned w[2] = {0, 0};
  HIPCK(h, hipMemcpy(w, h->d_plane_skip, sizeof(w), hipMemcpyDeviceToHost));
  if (last) *last = h->plane_calls ? (int)w[0] : 0;
  if (calls) *calls = h->plane_calls;
  if (reused) *reused = h->plane_calls ? (long)w[1] + (long)w[0] : 0;
  return 0;
}

int debug_set_teacher(dhw_handle* h, const float* reset_dev, float* capture_dev, int every) {
  if (!h) return DHW_ERR_ARG;
  if (every < 0 || (every > 0 && (!reset_dev || !capture_dev))) return fail(h, DHW_ERR_ARG, "dhw_debug_set_teacher: bad arguments");
  if (every != h->teach_every) plane_invalidate(h);   // (the python binding re-applies an unchanged setting before every sample call)
  h->teach_every = every;
  h->teach_reset = every ? reset_dev : nullptr;
  h->teach_capture = every ? capture_dev : nullptr;
  return 0;
}
