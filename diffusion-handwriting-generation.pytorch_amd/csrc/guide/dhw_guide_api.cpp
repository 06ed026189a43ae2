// dhw_guide_api.cpp — C-ABI of classifier-free guided sampling (include/dhw.h: dhw_guided_ddim_sample, dhw_guided_sample,
// dhw_guide_update).  Per step: ONE forward over 2B rows (sampler/sample.cpp: forward_enqueue) — rows [0, B) under the real
// condition, rows [B, 2B) under the guidance condition, the same x in both — then guide_update, eagerly on the caller's
// stream.  Nothing here touches h->d_seed, the sampler's staging buffers, its graph cache, its step plans or the plane tag.
#include <cstring>
#include <vector>

#include "../ddim/ddim.h"
#include "../sampler/denoiser.h"
#include "guide.h"

namespace {

// what the two sampling entries check alike, before the first HIP call (include/dhw.h, "Arguments"); the entry's own level / T
// checks run between the two halves
int guide_check_front(dhw_handle* h, const char* fn, const int64_t* text2, const float* style2, const float* out, int B, int L, int Lt, const int32_t* lens) {
  if (!text2 || !style2 || !out) return fail(h, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !text2 ? "text2" : !style2 ? "style2" : "out");
  return eager_check(h, fn, B, L, Lt, lens);
}
int guide_check_back(dhw_handle* h, const char* fn, const float* scale, int B, int L) {
  char msg[160];
  if (guide_check_scale(scale, B, msg, sizeof msg) || guide_check_capacity(B, h->dims.max_B, msg, sizeof msg) || guide_check_rows(B, L, msg, sizeof msg))
    return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  return 0;
}

// the scale stage (allocated once, never moved) and the copy of the call's scales into it, staged like the lengths
int stage_scale(dhw_handle* h, const float* scale, int B, hipStream_t st) {
  if (!h->d_guide_scale) {
    if (!h->h_guide_scale_pin) HIPCK(h, hipHostMalloc((void**)&h->h_guide_scale_pin, (size_t)h->dims.max_B * 4));
    if (!h->guide_ev) HIPCK(h, hipEventCreateWithFlags(&h->guide_ev, hipEventDisableTiming));
    if (int rc = dev_alloc(h, (void**)&h->d_guide_scale, (size_t)h->dims.max_B * 4)) return rc;
  }
  HIPCK(h, hipEventSynchronize(h->guide_ev));
  memcpy(h->h_guide_scale_pin, scale, (size_t)B * 4);
  HIPCK(h, hipMemcpyAsync(h->d_guide_scale, h->h_guide_scale_pin, (size_t)B * 4, hipMemcpyHostToDevice, st));
  HIPCK(h, hipEventRecord(h->guide_ev, st));
  return 0;
}

// The prologue behind the checks: dhw_finalize, the lengths of BOTH halves on the device, the scratch set, the scales.
int guide_begin(dhw_handle* h, int B, int L, int Lt, const int32_t* lens, const float* scale, void* hip_stream, EagerCall* ec) {
  std::vector<int32_t> lens2;
  if (lens) {
    lens2.assign(lens, lens + B);
    lens2.insert(lens2.end(), lens, lens + B);
  }
  int rc;
  if ((rc = eager_begin(h, 2 * B, L, Lt, lens ? lens2.data() : nullptr, hip_stream, ec)) || (rc = ensure_scratch(h))) return rc;
  return stage_scale(h, scale, B, ec->st);
}

// x(0) in both halves of the doubled state, sigma0 for all 2B rows; `copy` receives it once more (latent_out) or is null
int guide_start(dhw_handle* h, Ctx& c, hipStream_t st, const float* src, const int* dl, int B, int L, uint64_t seed, int64_t first_sample, float sigma0, float* copy) {
  const dhw_handle::DenoiseScratch& s = h->scratch;
  DdimStartParams sp{};
  sp.src = src;
  sp.src_cols = 2;
  sp.lens = dl;
  sp.rows = (long)B * L;
  sp.B = B;
  sp.L = L;
  sp.seed = seed;
  sp.first_sample = first_sample;
  sp.sigma0 = sigma0;
  for (int half = 0; half < 2; ++half) {
    sp.x = s.x + (size_t)half * sp.rows * 2;
    sp.sigma = s.sigma + (size_t)half * B;
    sp.copy = half == 0 ? copy : nullptr;
    RUN_SMALL(c, "ddim_start", launch_ddim_start(sp, st));
    if (c.err) return c.err;
  }
  return 0;
}

GuideParams guide_params(dhw_handle* h, const int* dl, int B, int L) {
  const dhw_handle::DenoiseScratch& s = h->scratch;
  GuideParams p{};
  p.x = s.x;
  p.eps = s.eps;
  p.pen = s.pen;
  p.lens = dl;
  p.scale = h->d_guide_scale;
  p.rows = (long)B * L;
  p.B = B;
  p.L = L;
  return p;
}

int sample_impl_guided_ddim(dhw_handle* h, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                            int S, const float* scale, const float* latent, uint64_t seed, int64_t first_sample, float* out, float* latent_out, void* hip_stream) {
  const char* fn = "dhw_guided_ddim_sample";
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  int rc = guide_check_front(h, fn, text2, style2, out, B, L, Lt, lens);
  if (rc) return rc;
  char msg[160];
  if (ddim_check_levels(T, levels, S, msg, sizeof msg)) return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  if ((rc = guide_check_back(h, fn, scale, B, L))) return rc;
  if (((uintptr_t)latent | (uintptr_t)latent_out) & 7)
    return fail(h, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)latent & 7) ? "latent" : "latent_out");

  EagerCall ec;
  if ((rc = guide_begin(h, B, L, Lt, lens, scale, hip_stream, &ec))) return rc;
  auto& [st, dl, c] = ec;   // the stream, the staged lengths (2B entries) or null, the Ctx of the small launches
  const dhw_handle::DenoiseScratch& s = h->scratch;
  const std::vector<DdimCoef> t = ddim_coef_table(schedule_abar(T).data(), levels, S);
  if ((rc = guide_start(h, c, st, latent, dl, B, L, seed, first_sample, t[0].A, latent_out))) return rc;

  GuideParams p = guide_params(h, dl, B, L);
  p.kind = GUIDE_DDIM;
  for (int j = 0; j < S; ++j) {
    if ((rc = forward_enqueue(h, s.x, text2, s.sigma, style2, 2 * B, L, Lt, s.eps, s.pen, st, dl))) return rc;
    const bool last = j == S - 1;
    p.c0 = t[(size_t)j].A;
    p.c1 = t[(size_t)j].B;
    p.c2 = t[(size_t)j + 1].A;
    p.c3 = t[(size_t)j + 1].B;
    p.out = last ? nullptr : s.x;
    p.out3 = last ? out : nullptr;
    p.sigma = last ? nullptr : s.sigma;
    p.sigma_next = p.c2;
    RUN_SMALL(c, "guide_update", launch_guide_update(p, st));
    if (c.err) return c.err;
  }
  return 0;
}

int sample_impl_guided(dhw_handle* h, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T, int mode, const float* scale,
                       const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream) {
  const char* fn = "dhw_guided_sample";
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  int rc = guide_check_front(h, fn, text2, style2, out, B, L, Lt, lens);
  if (rc) return rc;
  if (T < 1 || T > MAX_T) return fail(h, DHW_ERR_ARG, "%s: T = %d must lie in [1, 2^29]", fn, T);
  if (mode != 0 && mode != 1) return fail(h, DHW_ERR_ARG, "%s: mode = %d must be 0 (new) or 1 (standard)", fn, mode);
  if ((rc = guide_check_back(h, fn, scale, B, L))) return rc;
  if ((uintptr_t)noise & 7) return fail(h, DHW_ERR_ARG, "%s: noise must be 8-byte aligned", fn);

  EagerCall ec;
  if ((rc = guide_begin(h, B, L, Lt, lens, scale, hip_stream, &ec))) return rc;
  auto& [st, dl, c] = ec;
  const dhw_handle::DenoiseScratch& s = h->scratch;
  std::vector<float> beta, abar;
  schedule_host(T, beta, abar);
  const size_t step_stride = (size_t)B * L * 2;   // one noise draw for the whole batch
  if ((rc = guide_start(h, c, st, noise, dl, B, L, seed, first_sample, sqrtf(abar[(size_t)T - 1]), nullptr))) return rc;

  GuideParams p = guide_params(h, dl, B, L);
  p.kind = mode == 0 ? GUIDE_NEW : GUIDE_STANDARD;
  p.seed = seed;
  p.first_sample = first_sample;
  for (int k = 0, i = T - 1; i >= 0; --i, ++k) {
    if ((rc = forward_enqueue(h, s.x, text2, s.sigma, style2, 2 * B, L, Lt, s.eps, s.pen, st, dl))) return rc;
    const GuideStep g = guide_step(mode, beta.data(), abar.data(), i);
    const bool last = i == 0;
    p.c0 = g.c0;
    p.c1 = g.c1;
    p.c2 = g.c2;
    p.c3 = g.c3;
    p.add_noise = g.add_noise;
    p.z = noise ? noise + (size_t)(1 + k) * step_stride : nullptr;
    p.iter = k;
    p.out = last ? nullptr : s.x;
    p.out3 = last ? out : nullptr;
    p.sigma = last ? nullptr : s.sigma;
    p.sigma_next = g.sigma_next;
    RUN_SMALL(c, "guide_update", launch_guide_update(p, st));
    if (c.err) return c.err;
  }
  return 0;
}

int update_impl_guide(int kind, const float* base, const float* eps2, const float* pen, const int32_t* lens, const float* scale, const float* z, int B, int L, float c0,
                      float c1, float c2, float c3, float* out, float* out3, void* hip_stream) {
  const char* fn = "dhw_guide_update";
  char msg[160];
  if (guide_check_kind(kind, msg, sizeof msg) || guide_check_rows(B, L, msg, sizeof msg)) return fail(nullptr, DHW_ERR_ARG, "%s: %s", fn, msg);
  if (!base || !eps2 || !scale) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !base ? "base" : !eps2 ? "eps2" : "scale");
  if (!out && !out3) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (out and out3: one of them is needed)", fn);
  if (out3 && !pen) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (pen: out3 takes its third column from it)", fn);
  if (kind == GUIDE_DDIM && z) return fail(nullptr, DHW_ERR_ARG, "%s: z is given with kind = 0: the deterministic update adds no noise", fn);
  if (((uintptr_t)base | (uintptr_t)eps2 | (uintptr_t)z | (uintptr_t)out) & 7)
    return fail(nullptr, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)base & 7) ? "base" : ((uintptr_t)eps2 & 7) ? "eps2" : ((uintptr_t)z & 7) ? "z" : "out");
  if (((uintptr_t)lens | (uintptr_t)scale | (uintptr_t)pen | (uintptr_t)out3) & 3)
    return fail(nullptr, DHW_ERR_ARG, "%s: lens, scale, pen and out3 must be 4-byte aligned", fn);
  GuideParams p{};
  p.x = base;
  p.eps = eps2;
  p.pen = pen;
  p.lens = lens;
  p.scale = scale;
  p.z = z;
  p.rows = (long)B * L;
  p.B = B;
  p.L = L;
  p.kind = kind;
  p.c0 = c0;
  p.c1 = c1;
  p.c2 = c2;
  p.c3 = c3;
  p.add_noise = z != nullptr;
  p.out = out;
  p.out3 = out3;
  const hipError_t e = launch_guide_update(p, (hipStream_t)hip_stream);
  if (e != hipSuccess) return fail(nullptr, DHW_ERR_HIP, "%s: launch: %s", fn, hipGetErrorString(e));
  return 0;
}

}  // namespace

extern "C" {

int dhw_guided_ddim_sample(dhw_handle* h, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                           int S, const float* scale, const float* latent, uint64_t seed, int64_t first_sample, float* out, float* latent_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_guided_ddim_sample", int, {
    return sample_impl_guided_ddim(h, text2, style2, B, L, Lt, lens, T, levels, S, scale, latent, seed, first_sample, out, latent_out, hip_stream);
  });
}

int dhw_guided_sample(dhw_handle* h, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T, int mode, const float* scale,
                      const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_guided_sample", int, { return sample_impl_guided(h, text2, style2, B, L, Lt, lens, T, mode, scale, noise, seed, first_sample, out, hip_stream); });
}

int dhw_guide_update(int kind, const float* base, const float* eps2, const float* pen, const int32_t* lens, const float* scale, const float* z, int B, int L, float c0,
                     float c1, float c2, float c3, float* out, float* out3, void* hip_stream) {
  DHW_GUARD((dhw_handle*)nullptr, "dhw_guide_update", int, { return update_impl_guide(kind, base, eps2, pen, lens, scale, z, B, L, c0, c1, c2, c3, out, out3, hip_stream); });
}

}  // extern "C"
