// dhw_step_api.cpp — C-ABI of the eager samplers (include/dhw.h): deterministic sampling and inversion (dhw_ddim_sample,
// dhw_ddim_invert, dhw_ddim_update), classifier-free guided sampling (dhw_guided_ddim_sample,
// dhw_guided_sample, dhw_guide_update; §33) and the second-order multistep solver over the same levels (dhw_dpm_coefs,
// dhw_dpm_update, dhw_dpm_sample, dhw_guided_dpm_sample; §40) — one argument block, one kernel and one loop for all of them
// (§34, §41).  A sampling call is step_start, then per step the launches of dhw_forward /
// dhw_forward_ragged (sampler/sample.cpp: forward_enqueue) and one step_update (step_loop) — eagerly on the caller's stream.  A
// guided call runs ONE forward over 2B rows per step: rows [0, B) under the real condition, rows [B, 2B) under the guidance
// condition, the same x in both.  Nothing here touches h->d_seed, the sampler's staging buffers, its graph cache, its step
// plans or the plane tag.
#include <cstring>
#include <vector>

#include "../sampler/denoiser.h"
#include "solver_host.h"
#include "step.h"

namespace {

// ---------------------------------------------------------------- what every update hands to the one kernel
// what one step hands to step_update, computed on the host in fp32 before the first launch
struct Step {
  int kind;                                // StepKind
  float c0, c1, c2, c3;
  float sigma_next;                        // the next forward's sigma (a sampling loop; an update entry writes none)
  int add_noise = 0;                       // the ancestral kinds
  const float* z = nullptr;                // the step's external noise, or null
  int iter = 0;
  float k0 = 0, k1 = 0, c4 = 0, c5 = 0;    // STEP_DPM_SECOND (solver_host.h)
};

// a row of the solver's table as a step; the one place that turns solver_host.h's DpmKind (1 / 2: the row format of
// dhw_dpm_coefs) into a StepKind
Step dpm_step(const DpmCoef& c) { return Step{c.kind == DPM_SECOND ? STEP_DPM_SECOND : STEP_DPM_FIRST, c.c0, c.c1, c.c2, c.c3, c.c2, 0, nullptr, 0, c.k0, c.k1, c.c4, c.c5}; }

// the steps of a deterministic call: level j to level j + 1 of the coefficient table, no noise
std::vector<Step> ddim_steps(const std::vector<DdimCoef>& t, int S) {
  std::vector<Step> steps((size_t)S);
  for (size_t j = 0; j < (size_t)S; ++j) steps[j] = Step{STEP_DDIM, t[j].A, t[j].B, t[j + 1].A, t[j + 1].B, t[j + 1].A};
  return steps;
}

// the steps of a multistep call: the rows of the solver's table
std::vector<Step> dpm_steps(const std::vector<DpmCoef>& t) {
  std::vector<Step> steps(t.size());
  for (size_t j = 0; j < t.size(); ++j) steps[j] = dpm_step(t[j]);
  return steps;
}

// the block's per-call fields: the arrays, the shape, the halves; a multistep call passes its hist
StepParams step_params(const float* base, const float* eps, const float* pen, const int* lens, const float* scale, float* hist, int halves, int B, int L) {
  StepParams p{};
  p.base = base;
  p.eps = eps;
  p.pen = pen;
  p.lens = lens;
  p.scale = scale;
  p.hist = hist;
  p.rows = (long)B * L;
  p.B = B;
  p.L = L;
  p.halves = halves;
  return p;
}

// the block's per-step fields
void step_set(StepParams& p, const Step& g) {
  p.kind = g.kind;
  p.c0 = g.c0;
  p.c1 = g.c1;
  p.c2 = g.c2;
  p.c3 = g.c3;
  p.k0 = g.k0;
  p.k1 = g.k1;
  p.c4 = g.c4;
  p.c5 = g.c5;
  p.add_noise = g.add_noise;
  p.z = g.z;
  p.iter = g.iter;
  p.sigma_next = g.sigma_next;
}

// a handle-less update entry behind its checks: one launch on the caller's arrays
int update_launch(const char* fn, StepParams p, const Step& g, float* out, float* out3, void* hip_stream) {
  step_set(p, g);
  p.out = out;
  p.out3 = out3;
  const hipError_t e = launch_step_update(p, (hipStream_t)hip_stream);
  if (e != hipSuccess) return fail(nullptr, DHW_ERR_HIP, "%s: launch: %s", fn, hipGetErrorString(e));
  return 0;
}

// ---------------------------------------------------------------- the start and the loop of every sampling entry
// x(0) in every half of the state (one launch per half), sigma0 for all halves * B rows; `copy` receives it once more
// (latent_out) or is null
int step_start(dhw_handle* h, EagerCall& ec, int halves, const float* src, int src_cols, int B, int L, uint64_t seed, int64_t first_sample, float sigma0,
               float* copy) {
  auto& [st, dl, c] = ec;   // the stream, the staged lengths (halves * B entries) or null, the Ctx of the small launches (their profiling bracket)
  const dhw_handle::DenoiseScratch& s = h->scratch;
  DdimStartParams sp{};
  sp.src = src;
  sp.src_cols = src_cols;
  sp.lens = dl;
  sp.rows = (long)B * L;
  sp.B = B;
  sp.L = L;
  sp.seed = seed;
  sp.first_sample = first_sample;
  sp.sigma0 = sigma0;
  for (int half = 0; half < halves; ++half) {
    sp.x = s.x + (size_t)half * sp.rows * 2;
    sp.sigma = s.sigma + (size_t)half * B;
    sp.copy = half == 0 ? copy : nullptr;
    RUN_SMALL(c, "ddim_start", launch_ddim_start(sp, st));
    if (c.err) return c.err;
  }
  return 0;
}

// per step: the forward over halves * B rows, then the update in place; the last step writes the caller's [B, L, 3] instead.
// A call's steps are all multistep or none is: the first one decides the label and whether the block carries hist.
int step_loop(dhw_handle* h, EagerCall& ec, int halves, const int64_t* text, const float* style, int B, int L, int Lt, uint64_t seed, int64_t first_sample,
              const std::vector<Step>& steps, float* out) {
  auto& [st, dl, c] = ec;
  const dhw_handle::DenoiseScratch& s = h->scratch;
  const bool multistep = !steps.empty() && step_multistep(steps[0].kind);
  const char* label = multistep ? "dpm_update" : halves == 2 ? "guide_update" : "ddim_update";
  StepParams p = step_params(s.x, s.eps, s.pen, dl, halves == 2 ? h->d_guide_scale : nullptr, multistep ? s.hist : nullptr, halves, B, L);
  p.seed = seed;
  p.first_sample = first_sample;
  for (size_t j = 0; j < steps.size(); ++j) {
    if (int rc = forward_enqueue(h, s.x, text, s.sigma, style, halves * B, L, Lt, s.eps, s.pen, st, dl)) return rc;
    const bool last = j + 1 == steps.size();
    step_set(p, steps[j]);
    p.out = last ? nullptr : s.x;
    p.out3 = last ? out : nullptr;
    p.sigma = last ? nullptr : s.sigma;
    RUN_SMALL(c, label, launch_step_update(p, st));
    if (c.err) return c.err;
  }
  return 0;
}

// ---------------------------------------------------------------- deterministic sampling and inversion
// what dhw_ddim_sample and dhw_ddim_invert check alike, before the first HIP call (include/dhw.h, "Arguments")
int ddim_check_common(dhw_handle* h, const char* fn, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T,
                      const int32_t* levels, int S) {
  if (!text || !style) return fail(h, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !text ? "text" : "style");
  if (int rc = eager_check(h, fn, B, L, Lt, lens)) return rc;
  char msg[160];
  if (ddim_check_levels(T, levels, S, msg, sizeof msg)) return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  return 0;
}

// the multistep entries' own checks (behind the level checks, before the first HIP call) and their table
int dpm_check_table(dhw_handle* h, const char* fn, int T, const int32_t* levels, int S, int order, std::vector<DpmCoef>& table) {
  char msg[160];
  if (solver_check_order(order, msg, sizeof msg) || dpm_coef_table(schedule_abar(T).data(), levels, S, order, table, msg, sizeof msg))
    return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  return 0;
}

// the set's fifth buffer, behind ensure_scratch: allocated once, at the handle's capacity, never moved
int ensure_hist(dhw_handle* h) {
  if (h->scratch.hist) return 0;
  return dev_alloc(h, (void**)&h->scratch.hist, (size_t)h->dims.max_B * h->dims.max_L * 2 * 4);
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
  auto& [st, dl, c] = ec;
  const dhw_handle::DenoiseScratch& s = h->scratch;
  const std::vector<DdimCoef> t = ddim_coef_table(schedule_abar(T).data(), levels, S);
  if ((rc = step_start(h, ec, 1, strokes, 3, B, L, 0, 0, t[(size_t)S - 1].A, nullptr))) return rc;

  // the loop runs backwards: y(j+1) stays in scratch.x while the iterate w lives in scratch.w; the last iteration of a step
  // writes y(j) over it, the last one of the call writes the caller's latent_out
  StepParams p = step_params(s.x, s.eps, s.pen, dl, nullptr, nullptr, 1, B, L);
  p.kind = STEP_DDIM;
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
      RUN_SMALL(c, "ddim_update", launch_step_update(p, st));
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
  return update_launch(fn, step_params(base, eps, nullptr, lens, nullptr, nullptr, 1, B, L), Step{STEP_DDIM, c0, c1, c2, c3, 0.f}, out, nullptr, hip_stream);
}

// ---------------------------------------------------------------- guided sampling
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

// The four deterministic sampling entries.  halves = 1: dhw_ddim_sample / dhw_dpm_sample (text, style of B rows; scale is not
// read); halves = 2: dhw_guided_ddim_sample / dhw_guided_dpm_sample (text2, style2 of 2B rows).  order null: the ddim entries; else
// the dpm entries with that order.  Each entry keeps its own check order, messages and prologue.
int sample_impl_levels(dhw_handle* h, int halves, const int* order, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T,
                       const int32_t* levels, int S, const float* scale, const float* latent, uint64_t seed, int64_t first_sample, float* latent_out, float* out,
                       void* hip_stream) {
  const bool guided = halves == 2, dpm = order != nullptr;
  const char* fn = guided ? (dpm ? "dhw_guided_dpm_sample" : "dhw_guided_ddim_sample") : (dpm ? "dhw_dpm_sample" : "dhw_ddim_sample");
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  int rc;
  if (guided) {
    if ((rc = guide_check_front(h, fn, text, style, out, B, L, Lt, lens))) return rc;
    char msg[160];
    if (ddim_check_levels(T, levels, S, msg, sizeof msg)) return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  } else {
    if (!out) return fail(h, DHW_ERR_ARG, "%s: null pointer (out)", fn);
    if ((rc = ddim_check_common(h, fn, text, style, B, L, Lt, lens, T, levels, S))) return rc;
  }
  std::vector<DpmCoef> table;
  if (dpm && (rc = dpm_check_table(h, fn, T, levels, S, *order, table))) return rc;
  if (guided && (rc = guide_check_back(h, fn, scale, B, L))) return rc;
  if (((uintptr_t)latent | (uintptr_t)latent_out) & 7)
    return fail(h, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)latent & 7) ? "latent" : "latent_out");

  EagerCall ec;
  if (guided) rc = guide_begin(h, B, L, Lt, lens, scale, hip_stream, &ec);
  else if (!(rc = eager_begin(h, B, L, Lt, lens, hip_stream, &ec))) rc = ensure_scratch(h);   // (leaves dhw_sample's text plane alone: forward_enqueue)
  if (rc || (dpm && (rc = ensure_hist(h)))) return rc;
  const std::vector<Step> steps = dpm ? dpm_steps(table) : ddim_steps(ddim_coef_table(schedule_abar(T).data(), levels, S), S);
  if ((rc = step_start(h, ec, halves, latent, 2, B, L, seed, first_sample, steps[0].c0, latent_out))) return rc;   // (c0 of step 0 is A_0)
  return step_loop(h, ec, halves, text, style, B, L, Lt, 0, 0, steps, out);
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
  std::vector<float> beta, abar;
  schedule_host(T, beta, abar);
  const size_t step_stride = (size_t)B * L * 2;   // one noise draw for the whole batch
  std::vector<Step> steps((size_t)T);
  for (int k = 0, i = T - 1; i >= 0; --i, ++k) {
    const GuideStep g = guide_step(mode, beta.data(), abar.data(), i);
    steps[(size_t)k] = Step{mode == 0 ? STEP_NEW : STEP_STANDARD, g.c0, g.c1, g.c2, g.c3, g.sigma_next, g.add_noise, noise ? noise + (size_t)(1 + k) * step_stride : nullptr, k};
  }
  if ((rc = step_start(h, ec, 2, noise, 2, B, L, seed, first_sample, sqrtf(abar[(size_t)T - 1]), nullptr))) return rc;
  return step_loop(h, ec, 2, text2, style2, B, L, Lt, seed, first_sample, steps, out);
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
  return update_launch(fn, step_params(base, eps2, pen, lens, scale, nullptr, 2, B, L), Step{kind, c0, c1, c2, c3, 0.f, z != nullptr, z}, out, out3, hip_stream);
}

// ---------------------------------------------------------------- the multistep solver's handle-less entries
int coefs_impl_dpm(int T, const int32_t* levels, int S, int order, float* out) {
  const char* fn = "dhw_dpm_coefs";
  char msg[160];
  if (ddim_check_levels(T, levels, S, msg, sizeof msg) || solver_check_order(order, msg, sizeof msg)) return fail(nullptr, DHW_ERR_ARG, "%s: %s", fn, msg);
  if (!out) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (out)", fn);
  std::vector<DpmCoef> table;
  if (dpm_coef_table(schedule_abar(T).data(), levels, S, order, table, msg, sizeof msg)) return fail(nullptr, DHW_ERR_ARG, "%s: %s", fn, msg);
  for (int j = 0; j < S; ++j) dpm_row_pack(table[(size_t)j], out + (size_t)j * DPM_ROW);
  return 0;
}

int update_impl_dpm(const float* base, const float* eps, const float* pen, const int32_t* lens, const float* scale, float* hist, int B, int L, const float* coef,
                    float* out, float* out3, void* hip_stream) {
  const char* fn = "dhw_dpm_update";
  const int halves = scale ? 2 : 1;
  if (B < 1 || L < 1 || (long long)halves * B * L > 0x7fffffffLL)
    return fail(nullptr, DHW_ERR_ARG, "%s: shape out of range: B=%d L=%d (both >= 1, B * L below 2^31, 2 * B * L with a scale)", fn, B, L);
  if (!base || !eps || !hist || !coef)
    return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !base ? "base" : !eps ? "eps" : !hist ? "hist" : "coef");
  if (!out && !out3) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (out and out3: one of them is needed)", fn);
  if (out3 && !pen) return fail(nullptr, DHW_ERR_ARG, "%s: null pointer (pen: out3 takes its third column from it)", fn);
  DpmCoef c{};
  char msg[96];
  if (dpm_row_unpack(coef, c, msg, sizeof msg)) return fail(nullptr, DHW_ERR_ARG, "%s: %s", fn, msg);
  if (((uintptr_t)base | (uintptr_t)eps | (uintptr_t)hist | (uintptr_t)out) & 7)
    return fail(nullptr, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)base & 7) ? "base" : ((uintptr_t)eps & 7) ? "eps" : ((uintptr_t)hist & 7) ? "hist" : "out");
  if (((uintptr_t)lens | (uintptr_t)scale | (uintptr_t)pen | (uintptr_t)out3) & 3)
    return fail(nullptr, DHW_ERR_ARG, "%s: lens, scale, pen and out3 must be 4-byte aligned", fn);
  return update_launch(fn, step_params(base, eps, pen, lens, scale, hist, halves, B, L), dpm_step(c), out, out3, hip_stream);
}

}  // namespace

extern "C" {

int dhw_ddim_sample(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                    int S, const float* latent, uint64_t seed, int64_t first_sample, float* latent_out, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_ddim_sample", int, { return sample_impl_levels(h, 1, nullptr, text, style, B, L, Lt, lens, T, levels, S, nullptr, latent, seed, first_sample, latent_out, out, hip_stream); });
}

int dhw_ddim_invert(dhw_handle* h, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T,
                    const int32_t* levels, int S, int iters, float* latent_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_ddim_invert", int, { return invert_impl_ddim(h, strokes, text, style, B, L, Lt, lens, T, levels, S, iters, latent_out, hip_stream); });
}

int dhw_ddim_update(const float* base, const float* eps, const int32_t* lens, int B, int L, float c0, float c1, float c2, float c3, float* out,
                    void* hip_stream) {
  DHW_GUARD((dhw_handle*)nullptr, "dhw_ddim_update", int, { return update_impl_ddim(base, eps, lens, B, L, c0, c1, c2, c3, out, hip_stream); });
}

int dhw_guided_ddim_sample(dhw_handle* h, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                           int S, const float* scale, const float* latent, uint64_t seed, int64_t first_sample, float* out, float* latent_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_guided_ddim_sample", int, {
    return sample_impl_levels(h, 2, nullptr, text2, style2, B, L, Lt, lens, T, levels, S, scale, latent, seed, first_sample, latent_out, out, hip_stream);
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

int dhw_dpm_coefs(int T, const int32_t* levels, int S, int order, float* out) {
  DHW_GUARD((dhw_handle*)nullptr, "dhw_dpm_coefs", int, { return coefs_impl_dpm(T, levels, S, order, out); });
}

int dhw_dpm_update(const float* base, const float* eps, const float* pen, const int32_t* lens, const float* scale, float* hist, int B, int L, const float* coef,
                   float* out, float* out3, void* hip_stream) {
  DHW_GUARD((dhw_handle*)nullptr, "dhw_dpm_update", int, { return update_impl_dpm(base, eps, pen, lens, scale, hist, B, L, coef, out, out3, hip_stream); });
}

int dhw_dpm_sample(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                   int S, int order, const float* latent, uint64_t seed, int64_t first_sample, float* latent_out, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_dpm_sample", int, {
    return sample_impl_levels(h, 1, &order, text, style, B, L, Lt, lens, T, levels, S, nullptr, latent, seed, first_sample, latent_out, out, hip_stream);
  });
}

int dhw_guided_dpm_sample(dhw_handle* h, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T, const int32_t* levels,
                          int S, int order, const float* scale, const float* latent, uint64_t seed, int64_t first_sample, float* out, float* latent_out,
                          void* hip_stream) {
  DHW_GUARD(h, "dhw_guided_dpm_sample", int, {
    return sample_impl_levels(h, 2, &order, text2, style2, B, L, Lt, lens, T, levels, S, scale, latent, seed, first_sample, latent_out, out, hip_stream);
  });
}

}  // extern "C"
