// dhw_train_api.cpp — C-ABI of the training step (include/dhw_train.h): the loss / perturbation / optimizer / draw kernels of
// train.hip, the generic dhw_op_* operations of train/, and dhw_train_convblock — one ConvBlock forward + backward issued on those
// same generic launchers (strided GEMM, SiLU, FiLM backward), the way train_model.py's TrainModel._convblock chains them.
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dhw_train.h"
#include "abi_guard.h"
#include "dhw_kernels.h"
#include "host/device_arena.h"
#include "train/train_common.h"

namespace {

thread_local ErrBuf g_terr;   // per calling thread, as dhw_train_last_error() is documented

int tfail(int code, const char* fmt, ...) noexcept {
  va_list ap;
  va_start(ap, fmt);
  g_terr.vsetf(fmt, ap);
  va_end(ap);
  return code;
}
// the body of every extern "C" entry point runs inside this: no exception leaves the library (abi_guard.h)
#define TRAIN_GUARD(fn, R, ...) \
  return abi_guard<R>(fn, [&](const char* f_, const char* w_) { return tfail(DHW_ERR_INTERNAL, "%s: internal error: %s", f_, w_); }, [&]() -> R __VA_ARGS__)
#define THIP(call)                                                                            \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) return tfail(DHW_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));  \
  } while (0)

// scratch allocations of one dhw_train_convblock call, released on every exit path
struct Scratch {
  DeviceArena arena;
  ~Scratch() {
    hipDeviceSynchronize();
    arena.free_all();
  }
  float* f32(size_t n) {   // not zeroed
    void* p = nullptr;
    return arena.alloc(&p, n * sizeof(float), false) == hipSuccess ? (float*)p : nullptr;
  }
  float* upload(const float* host, size_t n) {
    float* p = nullptr;
    return arena.upload_f32(std::vector<float>(host, host + n), &p) == hipSuccess ? p : nullptr;
  }
};

// The three GEMMs of a Conv1d(k = 3, 'same' padding inside each sample of L rows) / nn.Linear (taps = 1) on C-last rows, W in torch
// layout [cout][cin][taps] — the descriptors Tape.conv3 / Tape.linear build (train_model.py).
// y[R, cout] = conv(x[R, cin]) + b
OpGemm fwd_gemm(const float* x, const float* W, const float* b, float* y, int R, int L, int cin, int cout, int taps) {
  OpGemm g{};
  g.A = x; g.sam = cin; g.sak = 1;
  g.B = W; g.sbk = taps; g.sbn = (long)cin * taps; g.sbt = 1;
  g.C = y; g.scm = cout; g.scn = 1;
  g.M = R; g.N = cout; g.K = taps * cin; g.nzo = g.nzi = 1; g.taps = taps; g.bias = b; g.alpha = 1.f;
  if (taps == 3) { g.a_shift = -1; g.a_tap_shift = 1; g.lr = L; }
  return g;
}
// dW[cout][cin][tap] += dy^T x[r + tap - 1] (the taps as the inner batch index), db += column sums of dy: both zeroed by the caller
OpGemm wgrad_gemm(const float* dy, const float* x, float* dW, float* db, int R, int L, int cin, int cout, int taps) {
  OpGemm g{};
  g.A = dy; g.sam = 1; g.sak = cout;
  g.B = x; g.sbk = cin; g.sbn = 1;
  g.C = dW; g.scm = (long)cin * taps; g.scn = taps; g.sczi = 1;
  g.M = cout; g.N = cin; g.K = R; g.nzo = 1; g.nzi = taps; g.taps = 1; g.alpha = 1.f; g.accumulate = 1; g.rowsum = db;
  if (taps == 3) { g.b_shift = -1; g.b_z_shift = 1; g.lr = L; }
  return g;
}
// dx[R, cin] (+)= sum_tap dy[r - (tap - 1)] W[:, :, tap], times SiLU'(dsilu_of) where the layer's input was SiLU(dsilu_of)
OpGemm dgrad_gemm(const float* dy, const float* W, float* dx, int accumulate, const float* dsilu_of, int R, int L, int cin, int cout, int taps) {
  OpGemm g{};
  g.A = dy; g.sam = cout; g.sak = 1;
  g.B = W; g.sbk = (long)cin * taps; g.sbn = taps; g.sbt = 1;
  g.C = dx; g.scm = cin; g.scn = 1;
  g.M = R; g.N = cin; g.K = taps * cout; g.nzo = g.nzi = 1; g.taps = taps; g.alpha = 1.f; g.accumulate = accumulate; g.dsilu_of = dsilu_of;
  if (taps == 3) { g.a_shift = 1; g.a_tap_shift = -1; g.lr = L; }
  return g;
}

}  // namespace

extern "C" {

const char* dhw_train_last_error(void) { return g_terr.c_str(); }

int dhw_train_perturb(const float* x, const float* eps, const float* alphas, int B, int L, float* out, void* hip_stream) {
  TRAIN_GUARD("dhw_train_perturb", int, {
    if (!x || !eps || !alphas || !out || B < 1 || L < 1) return tfail(DHW_ERR_ARG, "dhw_train_perturb: bad argument");
    THIP(launch_perturb(x, eps, alphas, B, L, out, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_train_loss(const float* eps, const float* score_pred, const float* pen, const float* pen_pred, const float* alphas, int B, int L,
                   float* out3, float* d_score, float* d_pen_pred, void* hip_stream) {
  TRAIN_GUARD("dhw_train_loss", int, {
    if (!eps || !score_pred || !pen || !pen_pred || !alphas || !out3 || B < 1 || L < 1) return tfail(DHW_ERR_ARG, "dhw_train_loss: bad argument");
    THIP(launch_loss(eps, score_pred, pen, pen_pred, alphas, B, L, out3, d_score, d_pen_pred, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_train_adam(int nbuf, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float max_norm, float* grad_norm_out, void* hip_stream) {
  TRAIN_GUARD("dhw_train_adam", int, {
    if (nbuf < 1 || !p || !g || !m || !v || !n || step < 1) return tfail(DHW_ERR_ARG, "dhw_train_adam: bad argument");
    hipStream_t st = (hipStream_t)hip_stream;
    // the squared-norm scalar: allocated once per DEVICE and kept for the life of the process (a hipMalloc / hipFree pair and a
    // stream synchronisation per update used to sit here).  One scalar per device: calls on different streams of one device must
    // not overlap, and the first call on a device allocates, so it must not be made under stream capture — dhw_train_adam_dev,
    // which takes the scalar from the caller, is the form for graphs and concurrent streams (include/dhw_train.h).
    static std::mutex sq_mu;
    static std::map<int, float*> sq_by_device;
    float* sq = nullptr;
    if (max_norm > 0.f || grad_norm_out) {
      int dev = 0;
      THIP(hipGetDevice(&dev));
      {
        std::lock_guard<std::mutex> lk(sq_mu);
        float*& slot = sq_by_device[dev];
        if (!slot) THIP(hipMalloc((void**)&slot, sizeof(float)));
        sq = slot;
      }
      THIP(hipMemsetAsync(sq, 0, sizeof(float), st));
      for (int i = 0; i < nbuf; ++i) THIP(launch_sqnorm(g[i], n[i], sq, st));
    }
    for (int i = 0; i < nbuf; ++i)
      THIP(launch_adam(p[i], g[i], m[i], v[i], n[i], lr, beta1, beta2, eps, weight_decay, step, max_norm > 0.f ? sq : nullptr, max_norm, st));
    if (sq && grad_norm_out) THIP(hipMemcpyAsync(grad_norm_out, sq, sizeof(float), hipMemcpyDeviceToDevice, st));   // (squared norm; stream-ordered)
    return 0;
  });
}

int dhw_train_convblock(int device, int B, int L, int cin, int cout, const float* x, const float* sigma, const float* dout,
                        const dhw_convblock_weights* w, float* out, float* dx, float* dsigma, const dhw_convblock_grads* g, void* hip_stream) {
  TRAIN_GUARD("dhw_train_convblock", int, {
    if (!x || !sigma || !dout || !w || !out || !dx || !dsigma || !g) return tfail(DHW_ERR_ARG, "dhw_train_convblock: null pointer");
    const int c1 = cout / 2;
    if (B < 1 || L < 2 || (L & 1) || cin % 32 || c1 % 32 || cout % 64) return tfail(DHW_ERR_ARG, "dhw_train_convblock: unsupported shape B=%d L=%d %d -> %d", B, L, cin, cout);
    const long rows = (long)B * L;
    // (the strided GEMM addresses its operands with 32-bit element offsets)
    if (rows * std::max(cin, cout) >= (1L << 31)) return tfail(DHW_ERR_ARG, "dhw_train_convblock: unsupported shape B=%d L=%d %d -> %d", B, L, cin, cout);
    THIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch s;
    const int R = (int)rows, tot = c1 + 2 * cout, cols = 2 * tot;   // FiLM table columns: gamma1|gamma2|gamma3|beta1|beta2|beta3
    const int go[3] = {0, c1, c1 + cout}, bo[3] = {tot, tot + c1, tot + c1 + cout};
    const size_t n1 = (size_t)c1 * cin * 3, n2 = (size_t)cout * c1 * 3, nf = (size_t)cout * cout, ns = (size_t)cout * cin * 3, nw = (size_t)cols * 32;

    // ---- weights as the caller holds them (torch layouts: the GEMM takes strides), activations kept for the backward pass
    float *w1 = s.upload(w->conv1_w, n1), *b1 = s.upload(w->conv1_b, c1), *w2 = s.upload(w->conv2_w, n2), *b2 = s.upload(w->conv2_b, cout);
    float *wfc = s.upload(w->fc_w, nf), *bfc = s.upload(w->fc_b, cout), *wsk = s.upload(w->skip_w, ns), *bsk = s.upload(w->skip_b, cout);
    float *wfilm = s.upload(w->film_w, nw), *bfilm = s.upload(w->film_b, cols);
    auto act = [&](int C) { return s.f32((size_t)rows * C); };
    float *xa = act(cin), *sk = act(cout), *u1 = act(c1), *h1 = act(c1), *u2 = act(cout), *h2 = act(cout), *u3 = act(cout);
    float *du3 = act(cout), *dh2 = act(cout), *du2 = act(cout), *dh1 = act(c1), *du1 = act(c1);
    float *film = s.f32((size_t)B * cols), *dfilm = s.f32((size_t)B * cols);
    if (!w1 || !b1 || !w2 || !b2 || !wfc || !bfc || !wsk || !bsk || !wfilm || !bfilm || !xa || !sk || !u1 || !h1 || !u2 || !h2 || !u3 || !du3 || !dh2 ||
        !du2 || !dh1 || !du1 || !film || !dfilm)
      return tfail(DHW_ERR_HIP, "dhw_train_convblock: out of device memory");
    // FiLM k (+ SiLU) (+ addend) of a GEMM's result as a further output of its pass
    auto rider = [&](OpGemm gm, int k, int silu, const float* addend, float* to) {
      gm.film_g = film + go[k]; gm.film_b = film + bo[k]; gm.film_ps = cols; gm.film_rows = L; gm.film_act = silu; gm.film_add = addend; gm.film_out = to;
      return gm;
    };
    auto film_bwd = [&](const float* dy, const float* u, int k, int C, int silu, float* du) {
      return launch_film_act_bwd(dy, u, film + go[k], film + bo[k], cols, B, L, C, silu, du, 0, dfilm + go[k], dfilm + bo[k], st);
    };

    // ---- forward (cnn.py:64-87) as TrainModel._convblock chains it: every affine rides on the GEMM in front of it
    THIP(launch_sgemm(fwd_gemm(sigma, wfilm, bfilm, film, B, 0, 32, cols, 1), st));
    THIP(launch_unary(0, x, rows * cin, xa, st));
    const OpGemm both[2] = {fwd_gemm(x, wsk, bsk, sk, R, L, cin, cout, 3), rider(fwd_gemm(xa, w1, b1, u1, R, L, cin, c1, 3), 0, 1, nullptr, h1)};
    THIP(launch_sgemm_group(both, 2, st));
    THIP(launch_sgemm(rider(fwd_gemm(h1, w2, b2, u2, R, L, c1, cout, 3), 1, 1, nullptr, h2), st));
    THIP(launch_sgemm(rider(fwd_gemm(h2, wfc, bfc, u3, R, 0, cout, cout, 1), 2, 0, sk, out), st));

    // ---- backward: weight gradient (bias gradient riding on it) and data gradient of a layer as a pair; both add into zeroed buffers
    THIP(hipMemsetAsync(g->conv1_w, 0, n1 * 4, st)); THIP(hipMemsetAsync(g->conv1_b, 0, c1 * 4, st));
    THIP(hipMemsetAsync(g->conv2_w, 0, n2 * 4, st)); THIP(hipMemsetAsync(g->conv2_b, 0, cout * 4, st));
    THIP(hipMemsetAsync(g->fc_w, 0, nf * 4, st));    THIP(hipMemsetAsync(g->fc_b, 0, cout * 4, st));
    THIP(hipMemsetAsync(g->skip_w, 0, ns * 4, st));  THIP(hipMemsetAsync(g->skip_b, 0, cout * 4, st));
    THIP(hipMemsetAsync(g->film_w, 0, nw * 4, st));  THIP(hipMemsetAsync(g->film_b, 0, cols * 4, st));
    THIP(hipMemsetAsync(dfilm, 0, (size_t)B * cols * 4, st));   // (film_act_bwd adds the per-sample gamma / beta gradients into it)
    // out = FiLM3(fc(h2)) + conv_skip(x): both branches see dout
    THIP(film_bwd(dout, u3, 2, cout, 0, du3));
    THIP(launch_sgemm_pair(wgrad_gemm(du3, h2, g->fc_w, g->fc_b, R, 0, cout, cout, 1), dgrad_gemm(du3, wfc, dh2, 0, nullptr, R, 0, cout, cout, 1), st));
    // h2 = SiLU(FiLM2(conv2(h1)))
    THIP(film_bwd(dh2, u2, 1, cout, 1, du2));
    THIP(launch_sgemm_pair(wgrad_gemm(du2, h1, g->conv2_w, g->conv2_b, R, L, c1, cout, 3), dgrad_gemm(du2, w2, dh1, 0, nullptr, R, L, c1, cout, 3), st));
    // h1 = SiLU(FiLM1(conv1(SiLU(x)))): the data gradient takes SiLU'(x) along and writes dx; the skip branch adds to it
    THIP(film_bwd(dh1, u1, 0, c1, 1, du1));
    THIP(launch_sgemm_pair(wgrad_gemm(du1, xa, g->conv1_w, g->conv1_b, R, L, cin, c1, 3), dgrad_gemm(du1, w1, dx, 0, x, R, L, cin, c1, 3), st));
    THIP(launch_sgemm_pair(wgrad_gemm(dout, x, g->skip_w, g->skip_b, R, L, cin, cout, 3), dgrad_gemm(dout, wsk, dx, 1, nullptr, R, L, cin, cout, 3), st));
    // the six FiLM Linears
    THIP(launch_sgemm_pair(wgrad_gemm(dfilm, sigma, g->film_w, g->film_b, B, 0, 32, cols, 1), dgrad_gemm(dfilm, wfilm, dsigma, 0, nullptr, B, 0, 32, cols, 1), st));
    THIP(hipStreamSynchronize(st));
    return 0;
  });
}

int dhw_train_adam_dev(int nbuf, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                       const float* hyper, float* sqnorm, void* hip_stream) {
  TRAIN_GUARD("dhw_train_adam_dev", int, {
    if (nbuf < 1 || !p || !g || !m || !v || !n || !hyper || !sqnorm) return tfail(DHW_ERR_ARG, "dhw_train_adam_dev: bad argument");
    hipStream_t st = (hipStream_t)hip_stream;
    THIP(hipMemsetAsync(sqnorm, 0, sizeof(float), st));
    for (int i = 0; i < nbuf; ++i) THIP(launch_sqnorm(g[i], n[i], sqnorm, st));
    for (int i = 0; i < nbuf; ++i) THIP(launch_adam_dev(p[i], g[i], m[i], v[i], n[i], hyper, sqnorm, st));
    return 0;
  });
}

int dhw_train_adam_ema_dev(int nbuf, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* ema,
                           const int64_t* n, const float* hyper, const float* ema_hyper, float* sqnorm, void* hip_stream) {
  TRAIN_GUARD("dhw_train_adam_ema_dev", int, {
    if (nbuf < 1) return tfail(DHW_ERR_ARG, "dhw_train_adam_ema_dev: nbuf = %d must be at least 1", nbuf);
    if (!ema) return tfail(DHW_ERR_ARG, "dhw_train_adam_ema_dev: ema is NULL");
    if (!ema_hyper) return tfail(DHW_ERR_ARG, "dhw_train_adam_ema_dev: ema_hyper is NULL");
    if (!p || !g || !m || !v || !n || !hyper || !sqnorm) return tfail(DHW_ERR_ARG, "dhw_train_adam_ema_dev: bad argument");
    for (int i = 0; i < nbuf; ++i)
      if (!p[i] || !g[i] || !m[i] || !v[i] || !ema[i] || n[i] < 0) return tfail(DHW_ERR_ARG, "dhw_train_adam_ema_dev: buffer %d has a NULL pointer or a negative size", i);
    hipStream_t st = (hipStream_t)hip_stream;
    THIP(hipMemsetAsync(sqnorm, 0, sizeof(float), st));
    for (int i = 0; i < nbuf; ++i) THIP(launch_sqnorm(g[i], n[i], sqnorm, st));
    for (int i = 0; i < nbuf; ++i) THIP(launch_adam_ema(p[i], g[i], m[i], v[i], ema[i], n[i], hyper, ema_hyper, sqnorm, st));
    return 0;
  });
}

int dhw_train_draw(const uint64_t* rng, int B, int L, float* eps, long long n_keep, int keep_per_sample, float p, float* keep, void* hip_stream) {
  TRAIN_GUARD("dhw_train_draw", int, {
    if (!rng || !eps || !keep || B < 1 || L < 1 || n_keep < 1 || keep_per_sample < 4 || keep_per_sample % 4 || n_keep % keep_per_sample || p < 0.f || p >= 1.f)
      return tfail(DHW_ERR_ARG, "dhw_train_draw: bad argument");
    THIP(launch_train_draw(rng, B, L, eps, n_keep, keep_per_sample, p, keep, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_train_batch_draw(const uint64_t* rng, int N, int B, const float* abar, int T, const int32_t* grp_start, const int32_t* grp_size,
                         const int32_t* grp_pos, const int32_t* members, int32_t* idx, int32_t* style_src, float* alphas, float* sigma, void* hip_stream) {
  TRAIN_GUARD("dhw_train_batch_draw", int, {
    if (N < 1) return tfail(DHW_ERR_ARG, "dhw_train_batch_draw: N = %d must be >= 1", N);
    if (B < 1) return tfail(DHW_ERR_ARG, "dhw_train_batch_draw: B = %d must be >= 1", B);
    if (T < 2) return tfail(DHW_ERR_ARG, "dhw_train_batch_draw: T = %d must be >= 2", T);
    const void* need[] = {rng, abar, idx, style_src, alphas, sigma};
    const char* names[] = {"rng", "abar", "idx", "style_src", "alphas", "sigma"};
    for (int i = 0; i < 6; ++i)
      if (!need[i]) return tfail(DHW_ERR_ARG, "dhw_train_batch_draw: %s is NULL", names[i]);
    const int given = !!grp_start + !!grp_size + !!grp_pos + !!members;
    if (given != 0 && given != 4) return tfail(DHW_ERR_ARG, "dhw_train_batch_draw: the group tables (grp_start, grp_size, grp_pos, members) are all NULL or all set");
    THIP(launch_batch_draw(rng, N, B, abar, T, grp_start, grp_size, grp_pos, members, idx, style_src, alphas, sigma, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_train_batch_gather(const float* strokes, const int64_t* text, const float* style, const int32_t* idx, const int32_t* style_src, int N, int B, int L,
                           int Lt, int S, float* x, float* pen, int64_t* ids, float* mask, float* style_out, void* hip_stream) {
  TRAIN_GUARD("dhw_train_batch_gather", int, {
    if (N < 1) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: N = %d must be >= 1", N);
    if (B < 1) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: B = %d must be >= 1", B);
    if (L < 8 || L % 8) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: L = %d must be a positive multiple of 8", L);
    if (Lt < 1) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: Lt = %d must be >= 1", Lt);
    if (S < 1) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: S = %d must be >= 1", S);
    const void* need[] = {strokes, text, style, idx, style_src, x, pen, ids, mask, style_out};
    const char* names[] = {"strokes", "text", "style", "idx", "style_src", "x", "pen", "ids", "mask", "style_out"};
    const unsigned align[] = {16, 8, 16, 4, 4, 16, 16, 8, 4, 16};   // the kernel moves style and stroke rows in 16-byte pieces, tokens in 8
    for (int i = 0; i < 10; ++i) {
      if (!need[i]) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: %s is NULL", names[i]);
      if ((uintptr_t)need[i] % align[i]) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: %s must be %u-byte aligned", names[i], align[i]);
    }
    const long long per = (long long)S * 320 + L / 4 + Lt;   // 16-byte pieces and tokens of one sample, one thread each
    if (per > 0x7fffff00LL || (per + 255) / 256 * B > 0x7fffffffLL) return tfail(DHW_ERR_ARG, "dhw_train_batch_gather: B * S = %d * %d is too large for one launch", B, S);
    THIP(launch_batch_gather(strokes, text, style, idx, style_src, N, B, L, Lt, S, x, pen, ids, mask, style_out, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_train_cond_drop(const uint64_t* rng, int B, int Lt, int S, float p, int64_t* ids, float* mask, float* style, int32_t* dropped, void* hip_stream) {
  TRAIN_GUARD("dhw_train_cond_drop", int, {
    if (B < 1) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: B = %d must be >= 1", B);
    if (Lt < 1) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: Lt = %d must be >= 1", Lt);
    if (S < 1) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: S = %d must be >= 1", S);
    if (!(p >= 0.f && p <= 1.f)) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: p = %g must lie in [0, 1]", (double)p);
    const void* need[] = {rng, ids, mask, style, dropped};
    const char* names[] = {"rng", "ids", "mask", "style", "dropped"};
    const unsigned align[] = {8, 8, 4, 16, 4};   // the kernel moves style rows in 16-byte pieces, tokens in 8
    for (int i = 0; i < 5; ++i) {
      if (!need[i]) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: %s is NULL", names[i]);
      if ((uintptr_t)need[i] % align[i]) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: %s must be %u-byte aligned", names[i], align[i]);
    }
    const long long per = (long long)S * 320 + Lt;   // 16-byte pieces and tokens of one sample, one thread each
    if (per > 0x7fffff00LL || (per + 255) / 256 * B > 0x7fffffffLL) return tfail(DHW_ERR_ARG, "dhw_train_cond_drop: B * S = %d * %d is too large for one launch", B, S);
    THIP(launch_cond_drop(rng, B, Lt, S, p, ids, mask, style, dropped, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_op_keep_mask(const uint64_t* rng, int site, long long n, int per_sample, float p, float* keep, void* hip_stream) {
  TRAIN_GUARD("dhw_op_keep_mask", int, {
    if (!rng || !keep || site < 3 || n < 1 || per_sample < 4 || per_sample % 4 || n % per_sample || p < 0.f || p >= 1.f)
      return tfail(DHW_ERR_ARG, "dhw_op_keep_mask: bad argument");
    THIP(launch_keep_mask(rng, site, n, per_sample, p, keep, (hipStream_t)hip_stream));
    return 0;
  });
}

int dhw_op_film_table(const float* sigma, const float* flat, const int64_t* woff, const int64_t* boff, int B, int total, float* film, void* hip_stream) {
  TRAIN_GUARD("dhw_op_film_table", int, {
    if (!sigma || !flat || !woff || !boff || !film || B < 1 || total < 1) return tfail(DHW_ERR_ARG, "dhw_op_film_table: bad argument");
    THIP(launch_film_table(0, sigma, flat, woff, boff, B, total, film, nullptr, nullptr, (hipStream_t)hip_stream));
    return 0;
  });
}
int dhw_op_film_table_bwd(const float* dfilm, const float* sigma, const float* flat, const int64_t* woff, const int64_t* boff, int B, int total,
                          float* grad_flat, float* dsigma, void* hip_stream) {
  TRAIN_GUARD("dhw_op_film_table_bwd", int, {
    if (!dfilm || !sigma || !flat || !woff || !boff || !grad_flat || !dsigma || B < 1 || total < 1)
      return tfail(DHW_ERR_ARG, "dhw_op_film_table_bwd: bad argument");
    THIP(launch_film_table(1, sigma, flat, woff, boff, B, total, const_cast<float*>(dfilm), grad_flat, dsigma, (hipStream_t)hip_stream));
    return 0;
  });
}

#define OPCHECK(cond, name) if (!(cond)) return tfail(DHW_ERR_ARG, name ": bad argument")

static int gemm_from_desc(const dhw_gemm_desc* d, OpGemm& g) {
  OPCHECK(d && d->A && d->B && d->C && d->M > 0 && d->N > 0 && d->K > 0 && d->nzo > 0 && d->nzi > 0 && d->lr >= 0 && d->taps >= 1, "dhw_op_gemm");
  if ((d->a_shift || d->b_shift || d->a_tap_shift || d->b_z_shift) && d->lr < 1) return tfail(DHW_ERR_ARG, "dhw_op_gemm: a shift needs lr (rows per sample)");
  if (d->taps > 1 && (d->K % d->taps || (d->K / d->taps) % 32)) return tfail(DHW_ERR_ARG, "dhw_op_gemm: taps > 1 needs K / taps to be a multiple of 32");
  g.A = d->A; g.sam = d->sam; g.sak = d->sak; g.sazo = d->sazo; g.sazi = d->sazi; g.a_shift = d->a_shift; g.a_tap_shift = d->a_tap_shift;
  g.B = d->B; g.sbk = d->sbk; g.sbn = d->sbn; g.sbzo = d->sbzo; g.sbzi = d->sbzi; g.sbt = d->sbt; g.b_shift = d->b_shift; g.b_z_shift = d->b_z_shift;
  g.C = d->C; g.scm = d->scm; g.scn = d->scn; g.sczo = d->sczo; g.sczi = d->sczi;
  g.M = d->M; g.N = d->N; g.K = d->K; g.nzo = d->nzo; g.nzi = d->nzi; g.lr = d->lr; g.taps = d->taps;
  g.bias = d->bias; g.alpha = d->alpha; g.accumulate = d->accumulate; g.bf16 = d->bf16 ? 1 : 0; g.rowsum = d->rowsum; g.addend = d->addend; g.act_out = d->act_out; g.dsilu_of = d->dsilu_of; g.stamps = nullptr;
  g.film_g = d->film_gamma; g.film_b = d->film_beta; g.film_ps = d->film_pstride; g.film_rows = d->film_rows; g.film_act = d->film_act; g.film_out = d->film_out; g.film_add = d->film_addend;
  if (g.film_out && (!g.film_g || !g.film_b || g.film_rows < 1 || g.accumulate)) return tfail(DHW_ERR_ARG, "dhw_op_gemm: film_out needs gamma, beta, film_rows >= 1 and accumulate = 0");
  // (the rider's second output and its addend are addressed without a batch offset, train/sgemm_core.h "unbatched GEMMs": every batch of a
  // batched launch would write the same film_out rows)
  if (g.film_out && (long long)g.nzo * g.nzi != 1) return tfail(DHW_ERR_ARG, "dhw_op_gemm: film_out is for unbatched GEMMs (nzo * nzi = 1), got %d x %d", g.nzo, g.nzi);
  return 0;
}
int dhw_op_gemm(const dhw_gemm_desc* d, void* hip_stream) {
  TRAIN_GUARD("dhw_op_gemm", int, {
    OpGemm g;
    if (int rc = gemm_from_desc(d, g)) return rc;
    THIP(launch_sgemm(g, (hipStream_t)hip_stream));
    return 0;
  });
}
int dhw_op_gemm2(const dhw_gemm_desc* d0, const dhw_gemm_desc* d1, void* hip_stream) {
  TRAIN_GUARD("dhw_op_gemm2", int, {
    OpGemm g0, g1;
    if (int rc = gemm_from_desc(d0, g0)) return rc;
    if (int rc = gemm_from_desc(d1, g1)) return rc;
    int nl = 2;
    THIP(launch_sgemm_pair(g0, g1, (hipStream_t)hip_stream, &nl));
    return nl;
  });
}
int dhw_op_gemm_group(const dhw_gemm_desc* d, int n, void* hip_stream) {
  TRAIN_GUARD("dhw_op_gemm_group", int, {
    OPCHECK(d && n >= 1 && n <= 6, "dhw_op_gemm_group");
    OpGemm g[6];
    for (int i = 0; i < n; ++i)
      if (int rc = gemm_from_desc(d + i, g[i])) return rc;
    int nl = n;
    THIP(launch_sgemm_group(g, n, (hipStream_t)hip_stream, &nl));
    return nl;
  });
}
int dhw_op_unary(int kind, const float* x, long long n, float* y, void* st) {
  TRAIN_GUARD("dhw_op_unary", int, {
    OPCHECK(x && y && n > 0 && (kind == 0 || kind == 1), "dhw_op_unary");
    THIP(launch_unary(kind, x, n, y, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_unary_bwd(int kind, const float* dy, const float* x, long long n, float* dx, int accumulate, void* st) {
  TRAIN_GUARD("dhw_op_unary_bwd", int, {
    OPCHECK(dy && x && dx && n > 0 && (kind == 0 || kind == 1), "dhw_op_unary_bwd");
    THIP(launch_unary_bwd(kind, dy, x, n, dx, accumulate, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_add(const float* a, const float* b, long long n, float* out, int accumulate, void* st) {
  TRAIN_GUARD("dhw_op_add", int, {
    OPCHECK(a && out && n > 0, "dhw_op_add");
    THIP(launch_add2(a, b, n, out, accumulate, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_add_rows(const float* x, const float* table, int B, int L, int C, float* out, void* st) {
  TRAIN_GUARD("dhw_op_add_rows", int, {
    OPCHECK(x && table && out && B > 0 && L > 0 && C > 0, "dhw_op_add_rows");
    THIP(launch_add_rows(x, table, (long)B * L * C, (long)L * C, out, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_film(const float* x, const float* gamma, const float* beta, long long pstride, int B, int L, int C, float* y, void* st) {
  TRAIN_GUARD("dhw_op_film", int, {
    OPCHECK(x && gamma && beta && y && B > 0 && L > 0 && C > 0, "dhw_op_film");
    THIP(launch_film_fwd(x, gamma, beta, pstride, B, L, C, y, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_film_bwd(const float* dy, const float* x, const float* gamma, long long pstride, int B, int L, int C, float* dx, int accumulate,
                    float* dgamma, float* dbeta, void* st) {
  TRAIN_GUARD("dhw_op_film_bwd", int, {
    OPCHECK(dy && x && gamma && dx && dgamma && dbeta && B > 0 && L > 0 && C > 0, "dhw_op_film_bwd");
    THIP(launch_film_bwd2(dy, x, gamma, pstride, B, L, C, dx, accumulate, dgamma, dbeta, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_film_act(const float* x, const float* gamma, const float* beta, long long pstride, int B, int L, int C, int act, const float* addend, float* y,
                    void* st) {
  TRAIN_GUARD("dhw_op_film_act", int, {
    // (the forward has the 16-byte kernel only: whole f32x4 per lane and aligned bases, addend included where it is given)
    OPCHECK(x && gamma && beta && y && B > 0 && L > 0 && C > 0 && C % 4 == 0 && pstride % 4 == 0 &&
                ((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)addend | (uintptr_t)y) % 16 == 0,
            "dhw_op_film_act");
    THIP(launch_film_act_fwd(x, gamma, beta, pstride, B, L, C, act, addend, y, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_film_act_bwd(const float* dy, const float* x, const float* gamma, const float* beta, long long pstride, int B, int L, int C, int act, float* dx,
                        int accumulate, float* dgamma, float* dbeta, void* st) {
  TRAIN_GUARD("dhw_op_film_act_bwd", int, {
    OPCHECK(dy && x && gamma && beta && dx && dgamma && dbeta && B > 0 && L > 0 && C > 0, "dhw_op_film_act_bwd");
    THIP(launch_film_act_bwd(dy, x, gamma, beta, pstride, B, L, C, act, dx, accumulate, dgamma, dbeta, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_ln_film(const float* x, int B, int L, int C, const float* gamma, const float* beta, long long pstride, const float* addend, float* y, float* act_out,
                   const float* pe, float* pe_out, float* mean, float* rstd, void* st) {
  TRAIN_GUARD("dhw_op_ln_film", int, {
    OPCHECK(x && gamma && beta && y && mean && rstd && B > 0 && L > 0 && C > 0 && (!pe_out || pe), "dhw_op_ln_film");
    THIP(launch_ln_film_fwd(x, (long)B * L, C, gamma, beta, pstride, L, addend, y, act_out, pe, pe_out, mean, rstd, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_ln_film_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, long long pstride, int B, int L, int C,
                       float* dx, int accumulate, float* dgamma, float* dbeta, void* st) {
  TRAIN_GUARD("dhw_op_ln_film_bwd", int, {
    OPCHECK(dy && x && mean && rstd && gamma && dx && dgamma && dbeta && B > 0 && L > 0 && C > 0 && C <= 512, "dhw_op_ln_film_bwd");
    THIP(launch_ln_film_bwd(dy, x, mean, rstd, gamma, pstride, B, L, C, dx, accumulate, dgamma, dbeta, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_layernorm(const float* x, long long rows, int C, float* y, float* mean, float* rstd, void* st) {
  TRAIN_GUARD("dhw_op_layernorm", int, {
    OPCHECK(x && y && mean && rstd && rows > 0 && C > 0, "dhw_op_layernorm");
    THIP(launch_ln_fwd(x, rows, C, y, mean, rstd, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_layernorm_bwd(const float* dy, const float* y, const float* rstd, long long rows, int C, float* dx, int accumulate, void* st) {
  TRAIN_GUARD("dhw_op_layernorm_bwd", int, {
    OPCHECK(dy && y && rstd && dx && rows > 0 && C > 0, "dhw_op_layernorm_bwd");
    THIP(launch_ln_bwd(dy, y, rstd, rows, C, dx, accumulate, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_softmax(const float* s, long long rows, int cols, long long rows_per_sample, const float* mask, float scale, float* p, void* st) {
  TRAIN_GUARD("dhw_op_softmax", int, {
    OPCHECK(s && p && rows > 0 && cols > 0 && rows_per_sample > 0, "dhw_op_softmax");
    THIP(launch_softmax_fwd(s, rows, cols, rows_per_sample, mask, scale, p, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_softmax_bwd(const float* dp, const float* p, long long rows, int cols, float scale, float* ds, void* st) {
  TRAIN_GUARD("dhw_op_softmax_bwd", int, {
    OPCHECK(dp && p && ds && rows > 0 && cols > 0, "dhw_op_softmax_bwd");
    THIP(launch_softmax_bwd(dp, p, rows, cols, scale, ds, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_resample(int mode, const float* x, long long rows_out, int C, float* y, int accumulate, void* st) {
  TRAIN_GUARD("dhw_op_resample", int, {
    OPCHECK(x && y && rows_out > 0 && C > 0 && mode >= 0 && mode <= 3, "dhw_op_resample");
    THIP(launch_pool(mode, x, rows_out * C, C, y, accumulate, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_embedding(const int64_t* ids, const float* table, long long rows, int C, float* y, void* st) {
  TRAIN_GUARD("dhw_op_embedding", int, {
    OPCHECK(ids && table && y && rows > 0 && C > 0, "dhw_op_embedding");
    THIP(launch_embed(0, ids, table, rows * C, C, y, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_embedding_bwd(const int64_t* ids, const float* dy, long long rows, int C, float* dtable, void* st) {
  TRAIN_GUARD("dhw_op_embedding_bwd", int, {
    OPCHECK(ids && dy && dtable && rows > 0 && C > 0, "dhw_op_embedding_bwd");
    THIP(launch_embed(1, ids, dy, rows * C, C, dtable, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_mask_mul(const float* x, const float* mask, float scale, long long n, float* y, int accumulate, void* st) {
  TRAIN_GUARD("dhw_op_mask_mul", int, {
    OPCHECK(x && mask && y && n > 0, "dhw_op_mask_mul");
    THIP(launch_mask_mul(x, mask, scale, n, y, accumulate, (hipStream_t)st));
    return 0;
  });
}
int dhw_op_colsum(const float* dy, long long rows, int C, float* db, void* st) {
  TRAIN_GUARD("dhw_op_colsum", int, {
    OPCHECK(dy && db && rows > 0 && C > 0, "dhw_op_colsum");
    THIP(launch_colsum(dy, rows, C, db, (hipStream_t)st));
    return 0;
  });
}

}  // extern "C"
