// dhw_api.cpp — the C-ABI of include/dhw.h and include/dhw_debug.h: every extern "C" entry point of the sampler, each a
// guarded call into the unit that does the work (sampler/handle.h maps them):
//   sampler/weights.cpp    state_dict inventory, padding, repacking into MFMA-fragment order (dhw_finalize)
//   sampler/workspace.cpp  activation workspaces, the all-steps text plane, teardown
//   sampler/denoiser.cpp   the denoiser launch sequence (== DiffusionModel.forward, reference model.py:121-182)
//   sampler/sample.cpp     dhw_forward, and the T-step sampler (== inference.py:80-96) with hipGraph replay
//   sampler/debug.cpp      debug, profiling and measurement hooks
// Here: the global error slot, dhw_create, the strict by-key intake.  No torch types, no exceptions across the ABI.
#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "host/error.h"
#include "plan/tile_plan.h"
#include "sampler/handle.h"
#include "xcd_swizzle.h"

static ErrBuf g_err;   // errors without a handle (dhw_create, dhw_schedule, dhw_render); a fixed buffer: recording an error never throws

void set_global_error(const char* fmt, va_list ap) noexcept { g_err.vsetf(fmt, ap); }

int fail(dhw_handle* h, int code, const char* fmt, ...) noexcept {
  va_list ap;
  va_start(ap, fmt);
  g_err.vsetf(fmt, ap);
  va_end(ap);
  if (h) h->err.set(g_err.c_str());
  return code;
}

// ================================================================= C-ABI
extern "C" {

const char* dhw_version(void) { return "dhw-hip 0.1 (gfx950)"; }

const char* dhw_last_error(dhw_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int dhw_schedule(int T, float* beta_out, float* alpha_bar_out) {
  DHW_GUARD(nullptr, "dhw_schedule", int, {
    if (T < 1 || !beta_out || !alpha_bar_out) return fail(nullptr, DHW_ERR_ARG, "dhw_schedule: bad args");
    std::vector<float> b, a;
    schedule_host(T, b, a);
    std::memcpy(beta_out, b.data(), T * 4);
    std::memcpy(alpha_bar_out, a.data(), T * 4);
    return 0;
  });
}

int dhw_create(dhw_handle** out, const dhw_dims* dims, int device) {
  DHW_GUARD(nullptr, "dhw_create", int, {
    if (!out || !dims) return fail(nullptr, DHW_ERR_ARG, "dhw_create: null argument");
    *out = nullptr;
    const dhw_dims& d = *dims;
    if (d.c1 != 128 || d.c3 != 256) return fail(nullptr, DHW_ERR_ARG, "c1 must be 128 and c3 256 (reference conditioning.py:9-10, model.py:103)");
    if (d.c2 < 12 || d.c2 > 192 || d.c2 % 12)
      return fail(nullptr, DHW_ERR_ARG, "c2 must be a multiple of 12 (model.py:88-106: 3 / 6 / 8 attention heads) and at most 192, the width the kernels are built for");
    if (d.num_layers < 0 || d.num_layers > 16 || d.max_B < 1 || d.max_L < 8 || d.max_L % 8 || d.max_Lt < 1 || d.S < 1 || (d.S * 1280) % STYLE_CH)
      return fail(nullptr, DHW_ERR_ARG, "dhw_create: bad dims");
    if (d.precision != DHW_PREC_BF16 && d.precision != DHW_PREC_F32) return fail(nullptr, DHW_ERR_ARG, "bad precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, DHW_ERR_HIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(nullptr, DHW_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
    // (owned here until the handle is complete: an exception on the way — caught by the guard — must not leak it)
    struct Hold {
      dhw_handle* p;
      ~Hold() { if (p) dhw_destroy(p); }
    } hold{new dhw_handle()};
    dhw_handle* h = hold.p;
    h->ldims = d;
    h->dims = d;
    h->dims.c2 = 192;
    h->padded = d.c2 != 192;
    h->device = device;
    h->prec = d.precision == DHW_PREC_F32 ? PREC_F32 : PREC_BF16;
    h->es = h->prec == PREC_F32 ? 4 : 2;
    h->store.init(build_spec(d.num_layers, d.c1, d.c2, d.c3));
    h->pspec = build_spec(d.num_layers, d.c1, h->dims.c2, d.c3);
    build_film_layout(h);
    build_names(h);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, DHW_ERR_HIP, "hipSetDevice failed");
    {
      const char* e = getenv("DHW_STREAMS");
      if (e && atoi(e) >= 1) h->nstreams = std::min(atoi(e), MAX_STREAMS);
      h->nstreams = std::max(1, std::min(h->nstreams, d.max_B));
      h->nstreams_alloc = h->nstreams;
    }
    int rc = alloc_shared(h);
    h->ws.resize(h->nstreams);
    // ws[0] serves dhw_forward at the full batch; the others only ever see ceil(max_B / nstreams) prompts
    for (int i = 0; !rc && i < h->nstreams; ++i)
      if (!(rc = alloc_workspace(h, h->ws[i], i == 0 ? d.max_B : (d.max_B + h->nstreams - 1) / h->nstreams))) rc = verify_workspace(h, h->ws[i]);
    for (int i = 1; !rc && i < h->nstreams; ++i)
      if (hipStreamCreateWithFlags(&h->sub_streams[i], hipStreamNonBlocking) != hipSuccess) rc = fail(h, DHW_ERR_HIP, "stream create failed");
    if (const char* e = getenv("DHW_FUSE")) h->fuse = atoi(e) != 0;
    if (const char* e = getenv("DHW_PLANE")) h->plane = atoi(e) != 0;
    if (const char* e = getenv("DHW_FUSE_TEXT")) h->fuse_text = atoi(e) != 0;
    if (const char* e = getenv("DHW_FUSE_HEADS")) h->fuse_heads = atoi(e) != 0;
    if (const char* e = getenv("DHW_FUSE_UP")) h->fuse_up = atoi(e) != 0;
    if (const char* e = getenv("DHW_CHAIN")) h->chain = atoi(e) != 0;
    if (const char* e = getenv("DHW_PERSIST")) h->persist = atoi(e) != 0;
    if (const char* e = getenv("DHW_PLANE_REUSE")) h->plane_reuse = atoi(e) != 0;
    if (const char* e = getenv("DHW_TEXT_PAIRS")) h->text_pairs = atoi(e) == 1 ? 1 : atoi(e) == 2 ? 2 : 0;
    if (const char* e = getenv("DHW_STORE_POLICY")) {
      const long v = strtol(e, nullptr, 0);
      bool ok = v >= 0 && v < 64;
      for (int cls = 0; ok && cls < 3; ++cls) ok = store_policy_of((int)v, cls) != 3;
      if (!ok && !rc) rc = fail(h, DHW_ERR_ARG, "DHW_STORE_POLICY=%s: two bits per output class (C, A, B from bit 0), each 0 = plain, 1 = write-through, 2 = early release", e);
      if (ok) h->store_policy = (int)v;
    }
    if (!rc && h->store_policy != DHW_STORE_DEFAULT && (enclayer_init_policy() != hipSuccess || convblock_init_policy() != hipSuccess))
      rc = fail(h, DHW_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(hipGetLastError()));
    if (h->padded) h->fuse = false;   // (pad_weights: the fused block kernels have compile-time LayerNorm widths)
    if (!rc && h->prec == PREC_BF16 && h->persist) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, device) != hipSuccess || persist_init() != hipSuccess) rc = fail(h, DHW_ERR_HIP, "persistent kernel setup failed: %s", hipGetErrorString(hipGetLastError()));
      else {
        h->persist_grid = prop.multiProcessorCount;
        if (hipHostMalloc((void**)&h->h_step_err, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void**)&h->d_step_err, h->h_step_err, 0) != hipSuccess)
          rc = fail(h, DHW_ERR_HIP, "host-mapped error word: %s", hipGetErrorString(hipGetLastError()));
        else *h->h_step_err = 0;
      }
    }
    if (!rc && enclayer_init() != hipSuccess) rc = fail(h, DHW_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && (enclayer_init_ragged() != hipSuccess || convblock_init_ragged() != hipSuccess || gemm_init_ragged() != hipSuccess))
      rc = fail(h, DHW_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && convblock_init() != hipSuccess) rc = fail(h, DHW_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && textside_init() != hipSuccess) rc = fail(h, DHW_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && gemm_init() != hipSuccess) rc = fail(h, DHW_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(hipGetLastError()));
    if (rc) { ErrBuf keep = h->err; g_err = keep; return rc; }   // (~Hold destroys the half-built handle; its message survives in the global slot)
    hold.p = nullptr;
    *out = h;
    return 0;
  });
}

void dhw_destroy(dhw_handle* h) {
  if (!h) return;
  try {
    destroy_impl(h);
  } catch (...) {   // (nothing below is expected to throw; the ABI's promise holds regardless)
  }
}

int dhw_num_keys(dhw_handle* h) { return h ? (int)h->store.spec.size() : DHW_ERR_ARG; }

int dhw_key_info(dhw_handle* h, int i, const char** key, int64_t shape[3], int* ndim) {
  DHW_GUARD(h, "dhw_num_keys", int, {
    if (!h || i < 0 || i >= (int)h->store.spec.size()) return fail(h, DHW_ERR_ARG, "dhw_key_info: index out of range");
    const KeySpec& k = h->store.spec[i];
    if (key) *key = k.key.c_str();
    if (ndim) *ndim = (int)k.shape.size();
    if (shape) for (size_t j = 0; j < 3; ++j) shape[j] = j < k.shape.size() ? k.shape[j] : 1;
    return 0;
  });
}

int dhw_load(dhw_handle* h, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  DHW_GUARD(h, "dhw_load", int, {
    if (!h || !key || !host_ptr || !shape) return fail(h, DHW_ERR_ARG, "dhw_load: null argument");
    switch (h->store.load(key, host_ptr, dtype, shape, ndim)) {
      case WeightStore::UNKNOWN_KEY: return fail(h, DHW_ERR_KEY, "unexpected key in state_dict: %s", key);
      case WeightStore::SIZE_MISMATCH: return fail(h, DHW_ERR_KEY, "size mismatch for %s", key);
      case WeightStore::BAD_DTYPE: return fail(h, DHW_ERR_ARG, "dhw_load: unknown dtype %d", dtype);
      case WeightStore::LOADED: break;
    }
    h->packed = false;
    plane_invalidate(h);   // (the next call's dhw_finalize repacks and counts a new weights generation)
    return 0;
  });
}

int dhw_finalize(dhw_handle* h) {
  DHW_GUARD(h, "dhw_finalize", int, { return finalize_impl(h); });
}

int dhw_forward(dhw_handle* h, const float* strokes, const int64_t* text, const float* sigma, const float* style,
                int B, int L, int Lt, float* eps_out, float* pen_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_forward", int, { return forward_impl(h, "dhw_forward", strokes, text, sigma, style, B, L, Lt, eps_out, pen_out, hip_stream, nullptr, false); });
}

int dhw_forward_ragged(dhw_handle* h, const float* strokes, const int64_t* text, const float* sigma, const float* style,
                       int B, int L, int Lt, const int32_t* lens, float* eps_out, float* pen_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_forward_ragged", int, { return forward_impl(h, "dhw_forward_ragged", strokes, text, sigma, style, B, L, Lt, eps_out, pen_out, hip_stream, lens, true); });
}

int dhw_sample(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, int T, int mode,
               const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_sample", int, { return sample_impl(h, "dhw_sample", text, style, B, L, Lt, T, mode, noise, seed, first_sample, out, hip_stream, nullptr, false); });
}

int dhw_sample_ragged(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T, int mode,
                      const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_sample_ragged", int, {
    return sample_impl(h, "dhw_sample_ragged", text, style, B, L, Lt, T, mode, noise, seed, first_sample, out, hip_stream, lens, true);
  });
}

int dhw_work(dhw_handle* h, int L, int Lt, double* flops_out, double* bytes_out) {
  DHW_GUARD(h, "dhw_work", int, { return work_impl(h, L, Lt, flops_out, bytes_out); });
}

// ---------------------------------------------------------------- debug / measurement hooks (sampler/debug.cpp)
int64_t dhw_debug_read(dhw_handle* h, const char* name, float* host_dst, int64_t max_floats, int64_t shape_out[3]) {
  DHW_GUARD(h, "dhw_debug_read", int64_t, { return debug_read(h, name, host_dst, max_floats, shape_out); });
}

int64_t dhw_debug_read_plane(dhw_handle* h, int workspace_slot, const char* name, float* host_dst, int64_t max_floats, int64_t shape_out[3]) {
  DHW_GUARD(h, "dhw_debug_read_plane", int64_t, { return debug_read_plane(h, workspace_slot, name, host_dst, max_floats, shape_out); });
}

int dhw_debug_xcd_swizzle(int block_id, int nwg) { return xcd_swizzle(block_id, nwg); }

int dhw_debug_raise(dhw_handle* h, int kind) {
  DHW_GUARD(h, "dhw_debug_raise", int, { return debug_raise(h, kind); });
}

int dhw_debug_randn(dhw_handle* h, uint64_t seed, int64_t first_sample, int B, int L, int iter, float* host_dst) {
  DHW_GUARD(h, "dhw_debug_xcd_swizzle", int, { return debug_randn(h, seed, first_sample, B, L, iter, host_dst); });
}

int dhw_debug_attention_time(dhw_handle* h, int layer, int iters, double* us_with, double* us_without, double* flops_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_debug_attention_time", int, { return debug_attention_time(h, layer, iters, us_with, us_without, flops_out, hip_stream); });
}

int dhw_profile_enable(dhw_handle* h, int on) {
  DHW_GUARD(h, "dhw_profile_enable", int, { return profile_enable(h, on); });
}
int dhw_profile_reset(dhw_handle* h) {
  DHW_GUARD(h, "dhw_profile_reset", int, { return profile_reset(h); });
}
int dhw_profile_count(dhw_handle* h) {
  DHW_GUARD(h, "dhw_profile_count", int, { return profile_count(h); });
}
int dhw_profile_get(dhw_handle* h, int i, const char** label, double* total_ms, int64_t* launches, double* flops_sum,
                    double* bytes_sum) {
  DHW_GUARD(h, "dhw_profile_get", int, { return profile_get(h, i, label, total_ms, launches, flops_sum, bytes_sum); });
}
int dhw_set_streams(dhw_handle* h, int n) {
  DHW_GUARD(h, "dhw_set_streams", int, { return set_streams(h, n); });
}
int dhw_debug_persist_plans(dhw_handle* h) {
  DHW_GUARD(h, "dhw_debug_persist_plans", int, { return debug_persist_plans(h); });
}
int dhw_debug_persist_trace(dhw_handle* h, unsigned long long* host_dst, int64_t max_words) {
  DHW_GUARD(h, "dhw_debug_persist_trace", int, { return debug_persist_trace(h, host_dst, max_words); });
}
int dhw_set_graph(dhw_handle* h, int on) {
  DHW_GUARD(h, "dhw_set_graph", int, { return set_graph(h, on); });
}
int dhw_debug_plane_reuse(dhw_handle* h, int* last, long* calls, long* reused) {
  DHW_GUARD(h, "dhw_debug_plane_reuse", int, { return debug_plane_reuse(h, last, calls, reused); });
}
int dhw_debug_plane_tag(const int64_t resident[10], const int64_t call[10], int gates) {
  DHW_GUARD(nullptr, "dhw_debug_plane_tag", int, {
    if (!resident || !call) return fail(nullptr, DHW_ERR_ARG, "dhw_debug_plane_tag: null argument");
    auto tag = [](const int64_t* v) {
      PlaneTag t;
      t.valid = v[0] != 0; t.B = (int)v[1]; t.nstreams = (int)v[2]; t.Lt = (int)v[3]; t.S = (int)v[4]; t.T = (int)v[5]; t.t_start = (int)v[6];
      t.weights_gen = (uint64_t)v[7]; t.film = (const void*)(uintptr_t)v[8]; t.plane_gen = (uint64_t)v[9];
      return t;
    };
    return (int)plane_host_ok(tag(resident), tag(call), PlaneGate{(gates & 1) != 0, (gates & 2) != 0, (gates & 4) != 0});
  });
}

// ---------------------------------------------------------------- the tile plan of the stroke kernels (plan/tile_plan.h), no device
int dhw_debug_conv_plan(int prec, int B, int L, int Cin, int Cout, int up_cin, int chain, const int64_t knobs[7], int out[12]) {
  DHW_GUARD(nullptr, "dhw_debug_conv_plan", int, {
    if (!knobs || !out || B < 1 || L < 1 || Cin < 0 || up_cin < 0) return fail(nullptr, DHW_ERR_ARG, "dhw_debug_conv_plan: bad args");
    ConvKnobs k;
    k.wgs = (long)knobs[0]; k.bm = (int)knobs[1]; k.occ = (int)knobs[2]; k.pp = (int)knobs[3];
    k.asym = knobs[4] != 0; k.tight = knobs[5] != 0; k.rt = knobs[6] != 0;
    const int i = out[0] = convblock_plan(prec, B, L, Cin, Cout, up_cin, chain != 0, k);
    if (i < 0) return 0;
    CONV_VARIANTS[i].row(out + 1);
    return 0;
  });
}

int dhw_debug_enc_plan(int prec, int d, int B, int Lk, int bm_min, const int64_t knobs[2], int out[4]) {
  DHW_GUARD(nullptr, "dhw_debug_enc_plan", int, {
    if (!knobs || !out || B < 1 || Lk < 1) return fail(nullptr, DHW_ERR_ARG, "dhw_debug_enc_plan: bad args");
    EncKnobs k;
    k.bm = (int)knobs[0]; k.wgs = (long)knobs[1];
    const EncVariant v{prec != PREC_BF16, d, enclayer_plan_bm(prec, d, B, Lk, bm_min, k)};
    out[0] = enc_find(v); out[1] = v.f32; out[2] = v.DM; out[3] = v.BM;
    return 0;
  });
}

int dhw_debug_gemm_plan(int prec, int B, int L, int N, int n_store, int ln, int out[2]) {
  DHW_GUARD(nullptr, "dhw_debug_gemm_plan", int, {
    if (!out || B < 1 || L < 1 || N < 1) return fail(nullptr, DHW_ERR_ARG, "dhw_debug_gemm_plan: bad args");
    GemmParams p{};
    p.B = B; p.L = L; p.N = N; p.n_store = n_store; p.ln = ln;
    gemm_tile_for(prec, p, &out[0], &out[1]);
    return 0;
  });
}

int dhw_debug_tile_knobs(int64_t out[12]) {
  DHW_GUARD(nullptr, "dhw_debug_tile_knobs", int, {
    if (!out) return fail(nullptr, DHW_ERR_ARG, "dhw_debug_tile_knobs: null argument");
    const ConvKnobs c = conv_knobs();
    const int64_t v[12] = {c.wgs, c.bm, c.occ, c.pp, c.asym, c.tight, c.rt, conv_stagger(0), enc_knobs(192).bm, enc_knobs(256).bm, enc_knobs(384).bm, enc_knobs(192).wgs};
    std::copy(v, v + 12, out);
    return 0;
  });
}

int dhw_debug_tile_variants(int kind, int i, int out[11]) {
  DHW_GUARD(nullptr, "dhw_debug_tile_variants", int, {
    if (kind != 0 && kind != 1) return fail(nullptr, DHW_ERR_ARG, "dhw_debug_tile_variants: kind must be 0 (ConvBlock) or 1 (EncoderLayer)");
    const int n = kind == 0 ? N_CONV_VARIANTS : N_ENC_VARIANTS;
    if (!out || i < 0 || i >= n) return n;   // (the length of the list alone)
    if (kind == 0) {
      CONV_VARIANTS[i].row(out);
    } else {
      const EncVariant& v = ENC_VARIANTS[i];
      out[0] = v.f32; out[1] = v.DM; out[2] = v.BM;
      enclayer_variant_facts(i, &out[3], &out[4]);
    }
    return n;
  });
}

int dhw_debug_set_teacher(dhw_handle* h, const float* reset_dev, float* capture_dev, int every) {
  DHW_GUARD(h, "dhw_debug_set_teacher", int, { return debug_set_teacher(h, reset_dev, capture_dev, every); });
}

}  // extern "C"
