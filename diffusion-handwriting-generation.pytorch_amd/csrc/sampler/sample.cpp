// sampler/sample.cpp — dhw_forward and the T-step sampler (== inference.py:80-96): the noise schedule, the per-T FiLM tables,
// ragged-length staging, the sampling loop with its hipGraph cache and persistent step plans, and dhw_work's operation count.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../cond/cond.h"
#include "denoiser.h"

int check_shapes(dhw_handle* h, int B, int L, int Lt, const char* fn) {
  const dhw_dims& d = h->dims;
  if (B < 1 || B > d.max_B || L < 8 || L > d.max_L || L % 8 || Lt < 1 || Lt > d.max_Lt)
    return fail(h, DHW_ERR_ARG, "%s%sshape out of range: B=%d (max %d) L=%d (max %d, multiple of 8) Lt=%d (max %d)", fn ? fn : "", fn ? ": " : "",
                B, d.max_B, L, d.max_L, Lt, d.max_Lt);
  return 0;
}

static int ensure_film_T(dhw_handle* h, int T, dhw_handle::FilmT** out) {
  dhw_handle::FilmT& ft = h->film_T[T];
  *out = &ft;
  if (ft.d_film) return 0;
  int rc;
  if ((rc = dev_alloc(h, (void**)&ft.d_sigma, (size_t)T * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&ft.d_sig32, (size_t)T * SIG * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&ft.d_film, (size_t)T * 2 * h->film_tot * 4))) return rc;
  return 0;
}

void schedule_host(int T, std::vector<float>& beta, std::vector<float>& alpha) {
  // utils/nn.py:19-39 in fp32: torch.linspace evaluates fma(step, i, start) below the midpoint and
  // fma(-step, n-1-i, end) above it (probed against torch 2.10 CPU); then exp, + 0.02,
  // cumprod(1 - beta) (inference.py:81).
  beta.resize(T);
  alpha.resize(T);
  const float lo = (float)std::log(1e-5), hi = (float)std::log(0.4);
  const float step = T > 1 ? (hi - lo) / (float)(T - 1) : 0.f;
  const int half = T / 2;
  double a = 1.0;   // torch's CPU cumprod accumulates float inputs in double (acc_type) and rounds each output
  for (int i = 0; i < T; ++i) {
    // (a one-point linspace is its START: torch.linspace(a, b, 1) = [a]; the symmetric form alone gave the end point for T = 1)
    const float x = T == 1 ? lo : i < half ? fmaf(step, (float)i, lo) : fmaf(-step, (float)(T - 1 - i), hi);
    beta[i] = 0.02f + expf(x);
    a = a * (double)(1.0f - beta[i]);
    alpha[i] = (float)a;
  }
}

std::vector<float> schedule_abar(int T) {
  std::vector<float> beta, abar;
  schedule_host(T, beta, abar);
  return abar;
}

// Ragged calls: check_lens checks the caller's lengths (host pointer, B entries) and refuses the diagnostic configurations that have
// no per-sample ends; stage_lens copies checked lengths into h->d_lens on the caller's stream.  The copy's source is the handle's pinned
// buffer, rewritten only once the previous call's copy has read it (an event on that copy, not a device-wide synchronize).
int check_lens(dhw_handle* h, const char* fn, const int32_t* lens, int B, int L, bool sampling) {
  if (!lens) return fail(h, DHW_ERR_ARG, "%s: lens is NULL (B = %d entries expected)", fn, B);
  for (int b = 0; b < B; ++b)
    if (lens[b] < 8 || lens[b] > L || lens[b] % 8)
      return fail(h, DHW_ERR_ARG, "%s: lens[%d] = %d: every length must be a multiple of 8 in [8, L = %d]", fn, b, (int)lens[b], L);
  if (sampling && h->persist) return fail(h, DHW_ERR_ARG, "%s: the persistent step kernel (DHW_PERSIST=1) does not support per-sample lengths", fn);
  return 0;
}

int stage_lens(dhw_handle* h, const int32_t* lens, int B, hipStream_t st) {
  HIPCK(h, hipEventSynchronize(h->lens_ev));
  memcpy(h->h_lens_pin, lens, (size_t)B * 4);
  HIPCK(h, hipMemcpyAsync(h->d_lens, h->h_lens_pin, (size_t)B * 4, hipMemcpyHostToDevice, st));
  HIPCK(h, hipEventRecord(h->lens_ev, st));
  return 0;
}

int eager_check(dhw_handle* h, const char* fn, int B, int L, int Lt, const int32_t* lens, bool name_shapes) {
  if (int rc = check_shapes(h, B, L, Lt, name_shapes ? fn : nullptr)) return rc;
  return lens ? check_lens(h, fn, lens, B, L, false) : 0;
}

// (plane reuse, DESIGN 27: the prologue writes h->d_lens alone — neither the all-steps plane nor the text / style staging buffers)
int eager_begin(dhw_handle* h, int B, int L, int Lt, const int32_t* lens, void* hip_stream, EagerCall* ec) {
  if (int rc = dhw_finalize(h)) return rc;
  HIPCK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (lens)
    if (int rc = stage_lens(h, lens, B, st)) return rc;
  *ec = EagerCall{st, lens ? h->d_lens : nullptr, Ctx{h, &h->ws[0], st, B, L, Lt, h->dims.S * 5, h->d_film, 0}};
  return 0;
}

int forward_impl(dhw_handle* h, const char* fn, const float* strokes, const int64_t* text, const float* sigma, const float* style,
                 int B, int L, int Lt, float* eps_out, float* pen_out, void* hip_stream, const int32_t* lens_host, bool ragged) {
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  if (!strokes || !text || !sigma || !style || !eps_out || !pen_out) return fail(h, DHW_ERR_ARG, "%s: null pointer", fn);
  int rc = eager_check(h, fn, B, L, Lt, lens_host);
  if (rc) return rc;
  if (ragged && !lens_host) return check_lens(h, fn, lens_host, B, L, false);   // (its message for a missing lens)
  EagerCall ec;
  if ((rc = eager_begin(h, B, L, Lt, lens_host, hip_stream, &ec))) return rc;
  return forward_enqueue(h, strokes, text, sigma, style, B, L, Lt, eps_out, pen_out, ec.st, ec.lens);
}

// The launches of one denoiser call on checked arguments (dhw_forward / dhw_forward_ragged, and every level of dhw_score);
// lens = the staged device lengths of a ragged call, or null.
// (plane reuse, DESIGN 27: the text side runs from the caller's own pointers into the per-call buffers ts / el[i].t of ws[0], planeT
// false and no skip word — the all-steps plane, the staging buffers and the plane tag are left alone by every entry built on this)
int forward_enqueue(dhw_handle* h, const float* strokes, const int64_t* text, const float* sigma, const float* style, int B, int L, int Lt,
                    float* eps_out, float* pen_out, hipStream_t st, const int* lens) {
  Ctx c{h, &h->ws[0], st, B, L, Lt, h->dims.S * 5, h->d_film, 2L * h->film_tot};
  c.lens = lens;
  taps_clear(h);
  RUN_SMALL(c, "sigma_ffn", launch_sigma_ffn(sigma, B, h->sg_w1, h->sg_b1, h->sg_w2, h->sg_b2, h->d_sig32, st));
  RUN_SMALL(c, "film_table", launch_film(h->d_sig32, B, h->d_film_w, h->d_film_b, 2 * h->film_tot, h->d_film, st));
  tap(c, TAP_SIGMA_FFN, h->d_sig32, 1, SIG, true);
  text_style_static(c, text, style);
  text_style_dynamic(c);   // (c.planeT false: always evaluated)
  stroke_path(c, strokes, text);
  HeadsParams hp{};
  hp.eps = eps_out;
  hp.pen = pen_out;
  launch_heads_for(c, hp);
  if (c.lens) {   // ragged: eps / pen past each sample's end are 0
    RUN_SMALL(c, "zero_tail", launch_zero_tail(eps_out, B, L, 2, c.lens, st));
    RUN_SMALL(c, "zero_tail", launch_zero_tail(pen_out, B, L, 1, c.lens, st));
  }
  h->last_B = B; h->last_L = L; h->last_Lt = Lt;
  return c.err;
}

// What is constant over one dhw_sample call: the shape, the library-owned staging buffers the call reads and writes, the
// schedule (T entries each), and the device lengths of a ragged call (or null).  A conditioned call (dhw_sample_cond) adds the
// staged known strokes (null = unconditioned), the keep mask and the conditioning noise (either may be null) and the number of
// iterations that run (t_start = T: all of them).
struct SampleCall {
  int B, L, Lt, T, mode;
  const int64_t* text;
  const float *style, *noise;
  float* out;
  const float *beta, *alpha;
  const int* lens;
  const float* known;
  const unsigned char* keep;
  const float* cond_noise;
  int t_start;
  int plane_call;   // profile mode: the slot of h_prof_skip that receives this call's plane-reuse flag, or -1
};

// One prompt sub-batch [b0, b0+Bs) of a B-prompt batch, enqueued on `st` with workspace `w`.
// d_plans: device array of T StepPlans (persist.h) -> every denoiser call is ONE persistent launch; rec_out: record mode —
// nothing is launched, the T plans are built on the host (rec_out->size() != T afterwards: this shape has no persistent form).
static int sample_enqueue(dhw_handle* h, const SampleCall& sc, Workspace* w, int b0, int Bs, hipStream_t st, const StepPlan* d_plans = nullptr,
                          std::vector<StepPlan>* rec_out = nullptr) {
  const int B = sc.B, L = sc.L, Lt = sc.Lt, T = sc.T, mode = sc.mode;
  const int64_t* text = sc.text;
  const float *style = sc.style, *noise = sc.noise, *alpha = sc.alpha, *beta = sc.beta;
  float* out = sc.out;
  const int* lens = sc.lens;
  const long rows = (long)Bs * L;
  const size_t step_stride = (size_t)B * L * 2;   // one noise draw for the whole batch
  text += (size_t)b0 * Lt;
  style += (size_t)b0 * h->dims.S * 1280;
  out += (size_t)b0 * L * 3;
  if (noise) noise += (size_t)b0 * L * 2;
  Ctx c{h, w, st, Bs, L, Lt, h->dims.S * 5, h->d_film_T, 0};
  c.fuse_input = true;
  c.lens = lens ? lens + b0 : nullptr;
  // x_T
  if (rec_out) {
  } else if (noise) {
    hipError_t e = hipMemcpyAsync(w->d_xt, noise, rows * 2 * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(h, DHW_ERR_HIP, "memcpy x_T: %s", hipGetErrorString(e));
  } else {
    RUN_SMALL(c, "randn_init", launch_randn_init(w->d_xt, rows, L, h->d_seed, b0, st));
  }
  // ragged: the padding rows of the sampler state start (and stay) 0 — nothing of a valid row reads them
  if (!rec_out && c.lens) RUN_SMALL(c, "zero_tail", launch_zero_tail(w->d_xt, Bs, L, 2, c.lens, st));
  // conditioned call: iterations [first, T) run; seeded rows start from the known strokes noised to schedule index t_start - 1
  const int first = T - sc.t_start;
  CondParams cp0{};
  if (sc.known) {
    cp0.x = w->d_xt;
    cp0.known = sc.known + (size_t)b0 * L * 3;
    cp0.keep = sc.keep ? sc.keep + (size_t)b0 * L : nullptr;
    cp0.lens = c.lens;
    cp0.rows = rows;
    cp0.L = L;
    cp0.seed_ptr = h->d_seed;
    cp0.sample_off = b0;
    if (!rec_out && (sc.keep || first > 0)) {
      CondParams cp = cp0;
      cp.ka = sqrtf(alpha[sc.t_start - 1]);
      cp.kb = sqrtf(1.0f - alpha[sc.t_start - 1]);
      RUN_SMALL(c, "cond_start", launch_cond_start(cp, first > 0, st));
    }
  }
  if (!rec_out) text_style_static(c, text, style);   // sigma-independent: once per sample batch, not per step
  const int TC = plane_chunk(T);
  for (int step = first, i = T - 1 - first; i >= 0; --i, ++step) {
    if (!rec_out && h->teach_every > 0 && step > first && step % h->teach_every == 0) {
      // teacher forcing (tests only): x after `step` steps -> capture[k], x := reset[k]
      const size_t k = (size_t)(step / h->teach_every - 1), off = (k * B + b0) * (size_t)L * 2;
      hipError_t e = hipMemcpyAsync(h->teach_capture + off, w->d_xt, rows * 2 * 4, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(w->d_xt, h->teach_reset + off, rows * 2 * 4, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return fail(h, DHW_ERR_HIP, "teacher copy: %s", hipGetErrorString(e));
    }
    if (!rec_out && h->plane && (step - first) % TC == 0) {   // (chunks are counted from the first iteration that runs)
      // The text side (TextStyleEncoder + every layer's text K/V, text_style.py:91-104, model.py:38-42) depends on
      // (text, style, sigma_i) only and the sigma schedule is known: evaluate it for the next `ns` steps in ONE
      // batched pass (ns*Bs "samples", FiLM row per step) instead of 16 small launches inside every step.
      const int ns = std::min(TC, T - step);
      Ctx cp = c;
      cp.B = ns * Bs;
      cp.in_B = Bs;
      cp.film = h->d_film_T + (size_t)i * 2 * h->film_tot;   // step `step + k` uses schedule index i - k
      cp.film_bs = -2L * h->film_tot;
      cp.film_div = Bs;
      cp.planeT = true;
      cp.plane_skip = h->d_plane_skip;   // resident and valid for this call: the launches return at once
      cp.plane_call = sc.plane_call;
      text_style_dynamic(cp);
      if (cp.err) return cp.err;
    }
    c.film = h->d_film_T + (size_t)i * 2 * h->film_tot;
    c.use_plane = h->plane;
    c.plane_step = (step - first) % TC;
    if (!h->plane) {
      if (rec_out) return 0;   // (the persistent form reads the text K/V from the all-steps plane)
      text_style_dynamic(c);   // (per step into the per-call buffers: no skip word)
    }
    HeadsParams hp{};
    hp.eps = nullptr;
    hp.pen = nullptr;
    hp.xt = w->d_xt;
    hp.z = noise ? noise + (size_t)(1 + step) * step_stride : nullptr;
    hp.mode = mode;
    hp.seed_ptr = h->d_seed;
    hp.sample_off = b0;
    hp.iter = step;
    const float a = alpha[i], b = beta[i];
    const float a_next = i > 1 ? alpha[i - 1] : 1.0f;   // inference.py:87
    hp.k0 = sqrtf(1.0f - a);
    if (mode == 0) {
      hp.k1 = sqrtf(1.0f - b);
      hp.k2 = sqrtf(1.0f - a_next);
      hp.add_noise = 1;
    } else {
      hp.k1 = 1.0f / sqrtf(1.0f - b);
      hp.k2 = sqrtf(b);
      hp.k3 = b;
      hp.add_noise = i != 0;   // inference.py:92
    }
    if (i == 0) hp.out3 = out;
    const bool fh = h->fuse && h->fuse_heads;
    c.fhp = fh ? &hp : nullptr;
    if (rec_out) {
      if (!fh) return 0;
      std::vector<StepPhase> phases;
      c.rec = &phases;
      c.rec_fail = false;
      stroke_path(c, w->d_xt, text);
      c.rec = nullptr;
      if (c.rec_fail || c.err || phases.empty()) return c.err;
      StepPlan sp{};
      sp.nphase = (int)phases.size();
      sp.B = Bs;
      sp.spx = (Bs + STEP_XCDS - 1) / STEP_XCDS;
      sp.sync = h->d_step_sync;
      sp.err = h->d_step_err;
      for (size_t k = 0; k < phases.size(); ++k) { sp.ph[k] = phases[k]; sp.cum_tps[k + 1] = sp.cum_tps[k] + phases[k].tps; }
      rec_out->push_back(sp);
      continue;
    }
    if (d_plans) {
      Launch l(h, st, "step.persistent");
      hipError_t e = launch_step(d_plans + step, h->persist_grid, st);
      if (e != hipSuccess) return fail(h, DHW_ERR_HIP, "persistent step %d: %s", step, hipGetErrorString(e));
      continue;
    }
    stroke_path(c, w->d_xt, text);
    if (!fh) launch_heads_for(c, hp);
    if (!fh && c.lens) RUN_SMALL(c, "zero_tail", launch_zero_tail(w->d_xt, Bs, L, 2, c.lens, st));   // (the stand-alone heads step every row)
    if (sc.keep) {
      // replacement conditioning: kept rows := the known strokes noised to the level this step arrived at, with the
      // conditioning stream's own draw (cond_noise[step], or the generator at iteration COND_ITER0 + step)
      CondParams cp = cp0;
      cp.ka = sqrtf(a_next);
      cp.kb = sqrtf(1.0f - a_next);
      cp.z = sc.cond_noise ? sc.cond_noise + (size_t)step * step_stride + (size_t)b0 * L * 2 : nullptr;
      cp.iter = COND_ITER0 + step;
      RUN_SMALL(c, "cond_replace", launch_cond_replace(cp, st));
    }
    if (c.err) return c.err;
  }
  // ragged: the output rows past each sample's end (the last step's tiles there exited without writing) are 0
  if (!rec_out && c.lens) RUN_SMALL(c, "zero_tail", launch_zero_tail(out, Bs, L, 3, c.lens, st));
  if (!rec_out && sc.keep) RUN_SMALL(c, "cond_finish", launch_cond_finish(out, cp0, st));   // kept rows of the output are `known`, pen included
  return c.err;
}

// The StepPlans of one dhw_sample shape (cached like the graphs): built by running the enqueue in record mode, uploaded once.
// Returns null when this shape / configuration has no persistent form (the caller then launches kernel by kernel).
// (only calls without per-sample lengths get here: sc.lens is null)
static const StepPlan* ensure_step_plans(dhw_handle* h, const std::vector<uint64_t>& key, const SampleCall& sc) {
  if (!h->persist || h->nstreams != 1 || h->prec != PREC_BF16 || !h->fuse || !h->plane || !h->fuse_heads || !h->fuse_up || !h->chain) return nullptr;
  auto it = h->plans.find(key);
  if (it != h->plans.end()) return it->second.ok ? it->second.dev : nullptr;
  dhw_handle::StepPlans& sp = h->plans[key];
  const size_t need = step_sync_words(sc.B);
  if (need > h->step_sync_words) {   // (earlier plans keep the smaller buffer: it is never freed before destroy)
    if (dev_alloc(h, (void**)&h->d_step_sync, need * sizeof(unsigned))) return nullptr;
    h->step_sync_words = need;
  }
  std::vector<StepPlan> host;
  if (sample_enqueue(h, sc, &h->ws[0], 0, sc.B, nullptr, nullptr, &host) || (int)host.size() != sc.T)
    return nullptr;
  if (getenv("DHW_PERSIST_TRACE") && atoi(getenv("DHW_PERSIST_TRACE"))) {
    if (!h->d_step_trace && dev_alloc(h, (void**)&h->d_step_trace, (size_t)h->persist_grid * STEP_MAX_PHASES * 4 * 8)) return nullptr;
    host.back().trace = h->d_step_trace;
  }
  if (dev_alloc(h, (void**)&sp.dev, host.size() * sizeof(StepPlan), false)) return nullptr;
  if (hipMemcpy(sp.dev, host.data(), host.size() * sizeof(StepPlan), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  sp.ok = true;
  return sp.dev;
}

// All sub-batches of one dhw_sample call.  On a capturing stream the sub-batches fork onto the handle's
// side streams (parallel graph branches) and join back; eagerly (profiling) they run one after another.
static int sample_enqueue_all(dhw_handle* h, const SampleCall& sc, bool fork, hipStream_t st, const StepPlan* d_plans = nullptr) {
  const int B = sc.B;
  const int ns = std::min(h->nstreams, B);
  const int per = (B + ns - 1) / ns;
  taps_clear(h);
  if (!fork || ns == 1) {
    for (int s = 0, b0 = 0; b0 < B; ++s, b0 += per) {
      int rc = sample_enqueue(h, sc, &h->ws[s], b0, std::min(per, B - b0), st, ns == 1 ? d_plans : nullptr);
      if (rc) return rc;
    }
    return 0;
  }
  hipEvent_t fork_ev, join_ev[MAX_STREAMS] = {};
  if (hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming) != hipSuccess) return fail(h, DHW_ERR_HIP, "event create failed");
  int rc = 0;
  if (hipEventRecord(fork_ev, st) != hipSuccess) rc = fail(h, DHW_ERR_HIP, "fork record failed");
  for (int s = 1, b0 = per; !rc && b0 < B; ++s, b0 += per) {
    hipStream_t ss = h->sub_streams[s];
    if (hipStreamWaitEvent(ss, fork_ev, 0) != hipSuccess) { rc = fail(h, DHW_ERR_HIP, "fork wait failed"); break; }
    rc = sample_enqueue(h, sc, &h->ws[s], b0, std::min(per, B - b0), ss);
    if (rc) break;
    if (hipEventCreateWithFlags(&join_ev[s], hipEventDisableTiming) != hipSuccess || hipEventRecord(join_ev[s], ss) != hipSuccess)
      rc = fail(h, DHW_ERR_HIP, "join record failed");
  }
  if (!rc) rc = sample_enqueue(h, sc, &h->ws[0], 0, std::min(per, B), st);
  for (int s = 1; s < MAX_STREAMS; ++s)
    if (join_ev[s]) {
      if (!rc && hipStreamWaitEvent(st, join_ev[s], 0) != hipSuccess) rc = fail(h, DHW_ERR_HIP, "join wait failed");
      hipEventDestroy(join_ev[s]);
    }
  hipEventDestroy(fork_ev);
  return rc;
}

// A staging buffer of `need` floats that cached graphs read (d_noise_stage, d_cond_noise_stage): growing it moves it, so the
// graphs and step plans that captured the old pointer are dropped first.
static int grow_stage(dhw_handle* h, float** buf, size_t* cap, size_t need) {
  if (need <= *cap) return 0;
  HIPCK(h, hipDeviceSynchronize());
  drop_graphs(h);
  h->plans.clear();
  if (int rc = dev_alloc(h, (void**)buf, need * 4, false)) return rc;
  *cap = need;
  return 0;
}

int sample_impl(dhw_handle* h, const char* fn, const int64_t* text, const float* style, int B, int L, int Lt, int T, int mode,
                const float* noise, uint64_t seed, int64_t first_sample, float* out, void* hip_stream, const int32_t* lens_host, bool ragged,
                const CondArgs* cond) {
  {
    if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
    if (!text || !style || !out) return fail(h, DHW_ERR_ARG, "%s: null pointer", fn);
    if (T < 1 || (mode != 0 && mode != 1)) return fail(h, DHW_ERR_ARG, "%s: bad T/mode", fn);
    int rc = check_shapes(h, B, L, Lt);
    if (rc) return rc;
    // (a conditioned call refuses the persistent step under its own name, below)
    if (ragged && (rc = check_lens(h, fn, lens_host, B, L, !cond))) return rc;
    if (cond) {
      // every check of the conditioned entry answers before the first HIP call (include/dhw.h, rules 5-7)
      if (h->persist) return fail(h, DHW_ERR_ARG, "%s: the persistent step kernel (DHW_PERSIST=1) does not support conditioned sampling", fn);
      if (cond->t_start < 1 || cond->t_start > T) return fail(h, DHW_ERR_ARG, "%s: t_start = %d must lie in [1, T = %d]", fn, cond->t_start, T);
      if (!cond->known && cond->keep) return fail(h, DHW_ERR_ARG, "%s: keep needs known (known is NULL)", fn);
      if (!cond->known && cond->t_start != T) return fail(h, DHW_ERR_ARG, "%s: t_start = %d < T = %d needs known (known is NULL)", fn, cond->t_start, T);
      if (cond->cond_noise && !(noise && cond->keep))
        return fail(h, DHW_ERR_ARG, "%s: cond_noise is given but %s: it belongs to calls with external noise and a keep mask", fn, noise ? "keep is NULL" : "noise is NULL");
      if (!cond->cond_noise && noise && cond->keep) return fail(h, DHW_ERR_ARG, "%s: cond_noise is NULL: a call with external noise and a keep mask needs it", fn);
      if (!cond->known) cond = nullptr;   // nothing is conditioned: the plain call, bit for bit (same graphs)
    }
    if ((rc = dhw_finalize(h))) return rc;
    HIPCK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (ragged && (rc = stage_lens(h, lens_host, B, st))) return rc;
    const int* lens = ragged ? h->d_lens : nullptr;
    if (h->h_step_err && *(volatile unsigned*)h->h_step_err) {
      // a persistent step kernel gave up waiting (bounded spin, persist.h): its results were wrong; say so and fall back for good
      const unsigned code = *(volatile unsigned*)h->h_step_err;
      *(volatile unsigned*)h->h_step_err = 0;
      h->persist = false;
      hipDeviceSynchronize();
      drop_graphs(h);   // (and with them the plane tag)
      if (h->d_step_sync) hipMemset(h->d_step_sync, 0, h->step_sync_words * sizeof(unsigned));
      if (code >= 0x100u)
        return fail(h, DHW_ERR_HIP, "persistent step kernel: XCD %u owns samples but no workgroup of the launch ran there in an EARLIER call (partitioned / "
                    "CU-masked device?): those samples were never computed; persistent launches are now disabled for this handle", code - 0x100u);
      return fail(h, DHW_ERR_HIP, "persistent step kernel timed out waiting for phase %u in an EARLIER call (its samples were invalid); "
                  "persistent launches are now disabled for this handle", code - 1);
    }
    dhw_handle::FilmT* ft = nullptr;
    if ((rc = ensure_film_T(h, T, &ft))) return rc;
    h->d_film_T = ft->d_film;
    if (h->plane) {
      const int ns = std::min(h->nstreams, B), per = (B + ns - 1) / ns;
      for (int s = 0; s < ns; ++s)
        if ((rc = ensure_plane(h, h->ws[s], plane_chunk(T), per))) return rc;
    }
    std::vector<float> beta, alpha;
    schedule_host(T, beta, alpha);
    if (!ft->ready) {
      // once per (weights, T): sigma_i = sqrt(abar_i) -> sigma MLP -> FiLM table [T, 2*TOT]; uploaded on the caller's
      // stream from a buffer the handle owns, so it is ordered against everything else this call enqueues
      ft->h_sigma.resize(T);
      for (int i = 0; i < T; ++i) ft->h_sigma[i] = sqrtf(alpha[i]);   // inference.py:89
      HIPCK(h, hipMemcpyAsync(ft->d_sigma, ft->h_sigma.data(), T * 4, hipMemcpyHostToDevice, st));
      Ctx c{h, &h->ws[0], st, B, L, Lt, h->dims.S * 5, ft->d_film, 0};
      RUN_SMALL(c, "sigma_ffn", launch_sigma_ffn(ft->d_sigma, T, h->sg_w1, h->sg_b1, h->sg_w2, h->sg_b2, ft->d_sig32, st));
      RUN_SMALL(c, "film_table", launch_film(ft->d_sig32, T, h->d_film_w, h->d_film_b, 2 * h->film_tot, ft->d_film, st));
      if (c.err) return c.err;
      ft->ready = true;
    }
    // the staging buffers that cached graphs read grow (dropping those graphs) before the reuse verdict below looks a graph up
    const size_t rows = (size_t)B * L;
    if (noise && (rc = grow_stage(h, &h->d_noise_stage, &h->noise_stage_cap, (size_t)(T + 1) * rows * 2))) return rc;
    if (cond && cond->cond_noise && (rc = grow_stage(h, &h->d_cond_noise_stage, &h->cond_noise_stage_cap, (size_t)T * rows * 2))) return rc;
    // Plane reuse: the host's half of the verdict.  The tag stays cleared until this call has been enqueued, so any
    // error return below leaves it cleared.  A graph keeps the ".T" buffers it was captured with: its generation is the one then.
    const bool graph = h->use_graph && !h->prof && !h->teach_every;
    const std::vector<uint64_t> key = {(uint64_t)B, (uint64_t)L, (uint64_t)Lt, (uint64_t)T, (uint64_t)mode, (uint64_t)(noise != nullptr), (uint64_t)h->nstreams, (uint64_t)h->plane, (uint64_t)h->fuse_heads, (uint64_t)h->fuse_up, (uint64_t)h->chain, (uint64_t)h->persist, (uint64_t)h->store_policy,
                                         (uint64_t)ragged,   // (ragged: the kernels read the lengths from h->d_lens at replay)
                                         // conditioned calls: known / keep / cond_noise are read from the staging buffers at replay,
                                         // so one graph serves every mask; the iterations it holds depend on t_start
                                         (uint64_t)(cond != nullptr), (uint64_t)(cond ? cond->t_start : T), (uint64_t)(cond && cond->keep), (uint64_t)(cond && cond->cond_noise)};
    PlaneTag call_tag;
    {
      auto gen = h->graph_plane_gen.find(key);
      call_tag.valid = true;
      call_tag.B = B; call_tag.nstreams = h->nstreams; call_tag.Lt = Lt; call_tag.S = h->dims.S; call_tag.T = T;
      call_tag.t_start = cond ? cond->t_start : T;
      call_tag.weights_gen = h->weights_gen;
      call_tag.film = ft->d_film;
      call_tag.plane_gen = graph && gen != h->graph_plane_gen.end() ? gen->second : h->plane_gen;
    }
    const PlaneGate gate{h->plane_reuse, h->plane, h->fuse && h->fuse_text && textside_supported(h->prec, Lt, h->dims.S * 5, 2 * h->dims.c2)};
    const unsigned host_ok = plane_host_ok(h->plane_tag, call_tag, gate);
    plane_invalidate(h);
    {
      hipError_t e = launch_set_seed(h->d_seed, seed, first_sample, st, h->d_plane_skip, host_ok);
      if (e != hipSuccess) return fail(h, DHW_ERR_HIP, "set_seed: %s", hipGetErrorString(e));
    }

    // stage the caller's prompts and styles into library-owned buffers (outside the graph); the same launch compares them with
    // what the stage held and clears the reuse flag on any difference
    {
      hipError_t e = launch_stage_compare(text, h->d_text_stage, (size_t)B * Lt * 8, style, h->d_style_stage, (size_t)B * h->dims.S * 1280 * 4, h->d_plane_skip, st);
      if (e != hipSuccess) return fail(h, DHW_ERR_HIP, "stage_compare: %s", hipGetErrorString(e));
    }
    int plane_call = -1;
    if (h->prof && h->h_prof_skip && h->prof_calls < dhw_handle::PROF_SKIP_CAP) {
      plane_call = h->prof_calls++;
      HIPCK(h, hipMemcpyAsync(h->h_prof_skip + plane_call, h->d_plane_skip, 4, hipMemcpyDeviceToHost, st));
    }
    const float* nz = nullptr;
    if (noise) {
      const size_t need = (size_t)(T + 1) * rows * 2;
      if ((rc = grow_stage(h, &h->d_noise_stage, &h->noise_stage_cap, need))) return rc;
      HIPCK(h, hipMemcpyAsync(h->d_noise_stage, noise, need * 4, hipMemcpyDeviceToDevice, st));
      nz = h->d_noise_stage;
    }
    const float *kn = nullptr, *cz = nullptr;
    const unsigned char* kp = nullptr;
    if (cond) {
      if (!h->d_known_stage) {   // (no cached graph reads these yet: only conditioned graphs do, and they are keyed apart)
        const size_t cap = (size_t)h->dims.max_B * h->dims.max_L;
        if ((rc = dev_alloc(h, (void**)&h->d_known_stage, cap * 3 * 4, false))) return rc;
        if ((rc = dev_alloc(h, (void**)&h->d_keep_stage, cap, false))) return rc;
      }
      HIPCK(h, hipMemcpyAsync(h->d_known_stage, cond->known, rows * 3 * 4, hipMemcpyDeviceToDevice, st));
      kn = h->d_known_stage;
      if (cond->keep) {
        HIPCK(h, hipMemcpyAsync(h->d_keep_stage, cond->keep, rows, hipMemcpyDeviceToDevice, st));
        kp = h->d_keep_stage;
      }
      if (cond->cond_noise) {
        const size_t need = (size_t)T * rows * 2;
        if ((rc = grow_stage(h, &h->d_cond_noise_stage, &h->cond_noise_stage_cap, need))) return rc;
        HIPCK(h, hipMemcpyAsync(h->d_cond_noise_stage, cond->cond_noise, need * 4, hipMemcpyDeviceToDevice, st));
        cz = h->d_cond_noise_stage;
      }
    }

    const SampleCall sc{B, L, Lt, T, mode, h->d_text_stage, h->d_style_stage, nz, h->d_out_stage, beta.data(), alpha.data(), lens,
                        kn, kp, cz, cond ? cond->t_start : T, plane_call};
    if (!graph) {
      // eager launches: sub-batches still fork onto the side streams (concurrent kernels of different sub-batches);
      // profiling keeps one stream so the per-launch events bracket one kernel each
      rc = sample_enqueue_all(h, sc, !h->prof, st);
    } else {
      auto it = h->graphs.find(key);
      if (it == h->graphs.end()) {
        const StepPlan* d_plans = ragged || kn ? nullptr : ensure_step_plans(h, key, sc);   // (before the capture: it uploads)
        hipStream_t cs;
        HIPCK(h, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) { hipStreamDestroy(cs); return fail(h, DHW_ERR_HIP, "begin capture: %s", hipGetErrorString(e)); }
        rc = sample_enqueue_all(h, sc, true, cs, d_plans);
        hipGraph_t g = nullptr;
        e = hipStreamEndCapture(cs, &g);
        if (rc == 0 && e != hipSuccess) rc = fail(h, DHW_ERR_HIP, "graph capture failed: %s", hipGetErrorString(e));
        hipGraphExec_t ex = nullptr;
        if (rc == 0) {
          e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
          if (e != hipSuccess) rc = fail(h, DHW_ERR_HIP, "graph instantiate failed: %s", hipGetErrorString(e));
        }
        if (g) hipGraphDestroy(g);
        hipStreamDestroy(cs);
        if (rc) return rc;
        it = h->graphs.emplace(key, ex).first;
        h->graph_plane_gen[key] = h->plane_gen;   // (== call_tag.plane_gen: no entry was found above)
      }
      HIPCK(h, hipGraphLaunch(it->second, st));
    }
    if (rc == 0) HIPCK(h, hipMemcpyAsync(out, h->d_out_stage, rows * 3 * 4, hipMemcpyDeviceToDevice, st));
    h->last_B = B; h->last_L = L; h->last_Lt = Lt;
    if (rc == 0) {   // enqueued: after this call the ".T" buffers hold the plane of call_tag (computed by it, or found valid)
      ++h->plane_calls;
      if (gate.plane && gate.text_fused) h->plane_tag = call_tag;
      // what dhw_debug_read_plane may copy out: every chunk writes from slot 0 on, so the longest chunk's slots were written
      const int ns = std::min(h->nstreams, B), per = (B + ns - 1) / ns;
      for (int s = 0; s < (int)h->ws.size(); ++s) {
        const int Bs = s < ns ? std::min(per, B - s * per) : 0;
        h->ws[s].plane_pairs = h->plane && Bs > 0 ? (long)plane_chunk(cond ? cond->t_start : T) * Bs : 0;
        h->ws[s].plane_Lt = Lt;
        h->ws[s].plane_last_gen = call_tag.plane_gen;
      }
    }
    return rc;
  }
}

int work_impl(dhw_handle* h, int L, int Lt, double* flops_out, double* bytes_out) {
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  const dhw_dims& d = h->ldims;   // the model's own widths: zero padding (pad_weights) is not algorithmic work
  const double c1 = d.c1, c2 = d.c2, c3 = d.c3, dt = 2 * c2, S5 = d.S * 5;
  auto cb = [](double L_, double ci, double co) { return 2 * L_ * (3 * ci * co + 1.5 * ci * co + 1.5 * co * co + co * co); };
  auto el = [&](double Lk, double dm, double heads) {
    double f = 2 * Lt * dt * dm + 2 * Lt * dm * dm * 2;            // text_dense, k1, v1
    f += 2 * Lk * dm * dm * 2 + 2 * Lk * dm * dm * 4;              // q1, dense1, qkv2, dense2
    f += 2 * Lk * dm * 2 * dm * 2;                                 // ffn
    f += 4 * Lk * Lt * dm + 4 * Lk * Lk * dm;                      // SDPA cross + self
    (void)heads;
    return f;
  };
  double f = 0;
  f += 2 * S5 * (STYLE_CH * 4 * c2 + 4 * c2 * dt) + 2 * Lt * dt * dt * 2 + 2 * S5 * dt * dt * 2 + 4 * Lt * S5 * dt + 2 * Lt * dt * 2 * dt * 2;
  f += 2 * L * 2 * c1;
  f += cb(L, c1, c1) + cb(L / 2, c1, c2) + cb(L / 4, c2, c3) + cb(L / 4, dt, c3) + cb(L / 2, c3, c2) + cb(L, c2, c1);
  f += el(L / 2, c2, 3) + el(L / 4, c3, 4) + d.num_layers * el(L / 8, dt, 6);
  f += 2 * (L / 8) * c3 * dt;
  f += 2 * 3 * ((L / 4) * c3 * dt + (L / 2) * c2 * c3 + L * c1 * c2);
  f += 2 * L * c1 * 3;
  // block-boundary activation bytes: every top-level block reads its inputs and writes its outputs once
  const double es = (double)h->es;
  double by = 0;
  by += L * 2 * 4 + L * 3 * 4;                                                  // strokes in, eps+pen out (fp32)
  by += es * (L * c1 * 2 + (L / 2) * (c1 + c2) + (L / 4) * (c2 + c3) + (L / 4) * (dt + c3) + (L / 2) * (c3 + c2) + L * (c2 + c1));   // ConvBlocks
  by += es * 2 * ((L / 2) * c2 + (L / 4) * c3 + d.num_layers * (L / 8) * dt);   // EncoderLayers
  by += es * ((L / 8) * (c3 + dt));                                             // att_dense
  by += es * ((L / 4) * (c3 + dt + dt) + (L / 2) * (c2 + c3 + c3) + L * (c1 + c2 + c2));   // skip convs + upsample add
  by += es * (S5 * STYLE_CH + Lt * dt * (2 + 2 * (2 + d.num_layers)));          // text/style encoder + per-layer text reads
  if (flops_out) *flops_out = f;
  if (bytes_out) *bytes_out = by;
  return 0;
}
