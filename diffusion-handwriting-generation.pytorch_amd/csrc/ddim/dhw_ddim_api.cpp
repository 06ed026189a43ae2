// dhw_ddim_api.cpp — C-ABI of deterministic sampling and inversion (include/dhw.h: dhw_ddim_sample, dhw_ddim_invert,
// dhw_ddim_update).  Per step: the launches of dhw_forward / dhw_forward_ragged (sampler/sample.cpp: forward_enqueue), then
// ddim_update — eagerly on the caller's stream.  Nothing here touches h->d_seed, the sampler's staging buffers, its graph
// cache or its step plans.
#include "../sampler/denoiser.h"
#include "ddim.h"

namespace {

// what dhw_ddim_sample and dhw_ddim_invert check alike, before the first HIP call (include/dhw.h, "Arguments")
int ddim_check_common(dhw_handle* h, const char* fn, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T,
                      const int32_t* levels, int S) {
  if (!text || !style) return fail(h, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !text ? "text" : "style");
  if (int rc = eager_check(h, fn, B, L, Lt, lens)) return rc;
  char msg[160];
  if (ddim_check_levels(T, levels, S, msg, sizeof msg)) return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  return 0;
}

int sample_impl_ddim(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                     int S, const float* latent, uint64_t seed, int64_t first_sample, float* latent_out, float* out, void* hip_stream) {
  const char* fn = "dhw_ddim_sample";
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  if (!out) return fail(h, DHW_ERR_ARG, "%s: null pointer (out)", fn);
  int rc = ddim_check_common(h, fn, text, style, B, L, Lt, lens, T, levels, S);
  if (rc) return rc;
  if (((uintptr_t)latent | (uintptr_t)latent_out) & 7)
    return fail(h, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)latent & 7) ? "latent" : "latent_out");

  EagerCall ec;
  if ((rc = eager_begin(h, B, L, Lt, lens, hip_stream, &ec)) || (rc = ensure_scratch(h))) return rc;   // (leaves dhw_sample's text plane alone: forward_enqueue)
  auto& [st, dl, c] = ec;   // the stream, the staged lengths or null, the Ctx of the small launches (their profiling bracket)
  const dhw_handle::DenoiseScratch& s = h->scratch;
  const std::vector<DdimCoef> t = ddim_coef_table(schedule_abar(T).data(), levels, S);

  DdimStartParams sp{};
  sp.src = latent;
  sp.src_cols = 2;
  sp.lens = dl;
  sp.rows = (long)B * L;
  sp.B = B;
  sp.L = L;
  sp.seed = seed;
  sp.first_sample = first_sample;
  sp.x = s.x;
  sp.copy = latent_out;
  sp.sigma = s.sigma;
  sp.sigma0 = t[0].A;
  RUN_SMALL(c, "ddim_start", launch_ddim_start(sp, st));
  if (c.err) return c.err;

  DdimParams p{};
  p.base = s.x;
  p.eps = s.eps;
  p.lens = dl;
  p.rows = sp.rows;
  p.B = B;
  p.L = L;
  p.pen = s.pen;
  for (int j = 0; j < S; ++j) {
    if ((rc = forward_enqueue(h, s.x, text, s.sigma, style, B, L, Lt, s.eps, s.pen, st, dl))) return rc;
    const bool last = j == S - 1;
    p.c0 = t[(size_t)j].A;
    p.c1 = t[(size_t)j].B;
    p.c2 = t[(size_t)j + 1].A;
    p.c3 = t[(size_t)j + 1].B;
    p.out = last ? nullptr : s.x;
    p.out3 = last ? out : nullptr;
    p.sigma = last ? nullptr : s.sigma;
    p.sigma_next = p.c2;
    RUN_SMALL(c, "ddim_update", launch_ddim_update(p, st));
    if (c.err) return c.err;
  }
  return 0;
}

int invert_impl_ddim(dhw_handle* h, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T,
                     const int32_t* levels, int S, int iters, float* latent_out, void* hip_stream) {
  const char* fn = "dhw_ddim_invert";
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  if (!strokes || !latent_out) return fail(h, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !strokes ? "strokes" : "latent_out");
  int rc = ddim_check_common(h, fn, text, style, B, L, Lt, lens, T, levels, S);
  if (rc) return rc;
  char msg[64];
  if (ddim_check_iters(iters, msg, sizeof msg)) return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  if ((uintptr_t)latent_out & 7) return fail(h, DHW_ERR_ARG, "%s: latent_out must be 8-byte aligned", fn);

  EagerCall ec;
  if ((rc = eager_begin(h, B, L, Lt, lens, hip_stream, &ec)) || (rc = ensure_scratch(h))) return rc;   // (leaves dhw_sample's text plane alone: forward_enqueue)
  auto& [st, dl, c] = ec;   // the stream, the staged lengths or null, the Ctx of the small launches (their profiling bracket)
  const dhw_handle::DenoiseScratch& s = h->scratch;
  const std::vector<DdimCoef> t = ddim_coef_table(schedule_abar(T).data(), levels, S);

  DdimStartParams sp{};
  sp.src = strokes;
  sp.src_cols = 3;
  sp.lens = dl;
  sp.rows = (long)B * L;
  sp.B = B;
  sp.L = L;
  sp.x = s.x;
  sp.sigma = s.sigma;
  sp.sigma0 = t[(size_t)S - 1].A;
  RUN_SMALL(c, "ddim_start", launch_ddim_start(sp, st));
  if (c.err) return c.err;

  // y(j+1) stays in scratch.x while the iterate w lives in scratch.w; the last iteration of a step writes y(j) over it, the last
  // one of the call writes the caller's latent_out
  DdimParams p{};
  p.base = s.x;
  p.eps = s.eps;
  p.lens = dl;
  p.rows = sp.rows;
  p.B = B;
  p.L = L;
  for (int j = S - 1; j >= 0; --j) {
    p.c0 = t[(size_t)j + 1].A;
    p.c1 = t[(size_t)j + 1].B;
    p.c2 = t[(size_t)j].A;
    p.c3 = t[(size_t)j].B;
    for (int k = 0; k < iters; ++k) {
      const float* w = k == 0 ? s.x : s.w;
      if ((rc = forward_enqueue(h, w, text, s.sigma, style, B, L, Lt, s.eps, s.pen, st, dl))) return rc;
      const bool step_done = k == iters - 1;
      p.out = !step_done ? s.w : j == 0 ? latent_out : s.x;
      p.sigma = step_done && j > 0 ? s.sigma : nullptr;
      p.sigma_next = j > 0 ? t[(size_t)j - 1].A : 0.f;
      RUN_SMALL(c, "ddim_update", launch_ddim_update(p, st));
      if (c.err) return c.err;
    }
  }
  return 0;
}

int update_impl_ddim(const float* base, const float* eps, const int32_t* lens, int B, int L, float c0, float c1, float c2, float c3, float* out,
                     void* hip_stream) {
  const char* fn = "dhw_ddim_update";
  if (B < 1 || L < 1 || (long long)B * L > 0x7fffffffLL)
    return fail(nullptr, DHW_ERR_ARG, "%s: shape out of range: B=%d L=%d (both >= 1, B * L below 2^31)", fn, B, L);
  if (!base || !eps || !out) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !base ? "base" : !eps ? "eps" : "out");
  if (((uintptr_t)base | (uintptr_t)eps | (uintptr_t)out) & 7)
    return fail(nullptr, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)base & 7) ? "base" : ((uintptr_t)eps & 7) ? "eps" : "out");
  if ((uintptr_t)lens & 3) return fail(nullptr, DHW_ERR_ARG, "%s: lens must be 4-byte aligned", fn);
  DdimParams p{};
  p.base = base;
  p.eps = eps;
  p.lens = lens;
  p.rows = (long)B * L;
  p.B = B;
  p.L = L;
  p.c0 = c0;
  p.c1 = c1;
  p.c2 = c2;
  p.c3 = c3;
  p.out = out;
  const hipError_t e = launch_ddim_update(p, (hipStream_t)hip_stream);
  if (e != hipSuccess) return fail(nullptr, DHW_ERR_HIP, "%s: launch: %s", fn, hipGetErrorString(e));
  return 0;
}

}  // namespace

extern "C" {

int dhw_ddim_sample(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                    int S, const float* latent, uint64_t seed, int64_t first_sample, float* latent_out, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_ddim_sample", int, { return sample_impl_ddim(h, text, style, B, L, Lt, lens, T, levels, S, latent, seed, first_sample, latent_out, out, hip_stream); });
}

int dhw_ddim_invert(dhw_handle* h, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T,
                    const int32_t* levels, int S, int iters, float* latent_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_ddim_invert", int, { return invert_impl_ddim(h, strokes, text, style, B, L, Lt, lens, T, levels, S, iters, latent_out, hip_stream); });
}

int dhw_ddim_update(const float* base, const float* eps, const int32_t* lens, int B, int L, float c0, float c1, float c2, float c3, float* out,
                    void* hip_stream) {
  DHW_GUARD((dhw_handle*)nullptr, "dhw_ddim_update", int, { return update_impl_ddim(base, eps, lens, B, L, c0, c1, c2, c3, out, hip_stream); });
}

}  // extern "C"
