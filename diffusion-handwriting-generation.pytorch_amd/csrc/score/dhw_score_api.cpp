// dhw_score_api.cpp — C-ABI of scoring (include/dhw.h: dhw_score): the denoising objective of given strokes at K noise
// levels.  Per level: score_perturb, the launches of dhw_forward_ragged (sampler/sample.cpp: forward_enqueue), score_reduce —
// eagerly on the caller's stream.  Nothing here touches h->d_seed, the sampler's staging buffers or its graph cache.
#include "../sampler/denoiser.h"
#include "score.h"

static int score_impl(dhw_handle* h, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens,
                      int T, const int32_t* levels, int K, const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream) {
  const char* fn = "dhw_score";
  // every check answers before the first HIP call (include/dhw.h, rule 7)
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  if (!strokes || !text || !style || !out) return fail(h, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !strokes ? "strokes" : !text ? "text" : !style ? "style" : "out");
  int rc = eager_check(h, fn, B, L, Lt, lens);
  if (rc) return rc;
  char msg[128];
  if (score_check_levels(T, levels, K, msg, sizeof msg)) return fail(h, DHW_ERR_ARG, "%s: %s", fn, msg);
  if (((uintptr_t)out | (uintptr_t)noise) & 7) return fail(h, DHW_ERR_ARG, "%s: %s must be 8-byte aligned", fn, ((uintptr_t)out & 7) ? "out" : "noise");

  EagerCall ec;
  if ((rc = eager_begin(h, B, L, Lt, lens, hip_stream, &ec)) || (rc = ensure_scratch(h))) return rc;   // (leaves dhw_sample's text plane alone: forward_enqueue)
  auto& [st, dl, c] = ec;   // the stream, the staged lengths or null, the Ctx of the two small launches (their profiling bracket)
  const dhw_handle::DenoiseScratch& s = h->scratch;   // x = x_t, w = the draw z
  const std::vector<ScoreLevel> table = score_level_table(schedule_abar(T).data(), levels, K);

  ScoreParams p{};
  p.strokes = strokes;
  p.lens = dl;
  p.rows = (long)B * L;
  p.B = B;
  p.L = L;
  p.seed = seed;
  p.first_sample = first_sample;
  p.xt = s.x;
  p.sigma = s.sigma;
  p.z = s.w;
  p.eps = s.eps;
  p.pen = s.pen;
  for (int k = 0; k < K; ++k) {
    p.lv = table[(size_t)k];
    p.noise = noise ? noise + (size_t)k * p.rows * 2 : nullptr;
    p.out = out + (size_t)k * B * 2;
    RUN_SMALL(c, "score_perturb", launch_score_perturb(p, st));
    if (c.err) return c.err;
    if ((rc = forward_enqueue(h, p.xt, text, p.sigma, style, B, L, Lt, s.eps, s.pen, st, p.lens))) return rc;
    RUN_SMALL(c, "score_reduce", launch_score_reduce(p, st));
    if (c.err) return c.err;
  }
  return 0;
}

extern "C" {

int dhw_score(dhw_handle* h, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens,
              int T, const int32_t* levels, int K, const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_score", int, { return score_impl(h, strokes, text, style, B, L, Lt, lens, T, levels, K, noise, seed, first_sample, out, hip_stream); });
}

}  // extern "C"
