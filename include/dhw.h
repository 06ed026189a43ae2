/* dhw.h — C-ABI of libdhw_hip.so: the MI355X (gfx950) reverse-diffusion
 * handwriting sampler.
 *
 * The reference (sleep3r/Diffusion-Handwriting-Generation.pytorch) is pure
 * Python and has no FFI; the hot path sits behind two Python surfaces, which
 * these entry points replace one-to-one (paths relative to
 * diffusion_handwriting_generation/ in the reference):
 *
 *   dhw_create / dhw_load / dhw_finalize
 *        <- DiffusionModel.__init__ (model.py:64-119) + strict state_dict load
 *           (checkpoint.py:92-130): weight interchange is the reference's own
 *           state_dict, key by key, torch-native layouts.
 *   dhw_forward  <- DiffusionModel.forward (model.py:121-182)
 *   dhw_sample   <- the T-step loop inlined in infer() (inference.py:80-96),
 *                   incl. get_beta_set (utils/nn.py:19-39) and the step
 *                   functions (utils/nn.py:64-112)
 *   dhw_schedule <- get_beta_set + cumprod (utils/nn.py:19-39, inference.py:81)
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every function
 * returns 0 on success or a negative dhw_status; nothing throws across the
 * ABI: every entry point of this library (dhw.h, dhw_debug.h, dhw_style.h,
 * dhw_train.h) runs inside a catch-all barrier that turns a C++ exception into
 * DHW_ERR_INTERNAL + a message (tests/test_host_cpu.py provokes one).  All tensor arguments of dhw_forward / dhw_sample are DEVICE pointers to
 * contiguous row-major buffers owned by the caller; work is enqueued on the
 * given HIP stream and is asynchronous w.r.t. the host.  The library owns its
 * packed weights, FiLM tables and workspace (sized at create from the dims).
 * One handle per device; a handle is not re-entrant (one in-flight call);
 * different handles are independent (batch shards across GPUs use one each).
 */
#ifndef DHW_H
#define DHW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dhw_handle dhw_handle;

typedef enum {
  DHW_OK = 0,
  DHW_ERR_ARG = -1,       /* bad argument / unsupported dims */
  DHW_ERR_KEY = -2,       /* unknown, duplicate or missing state_dict key, or shape mismatch */
  DHW_ERR_HIP = -3,       /* HIP runtime error (no device, launch failure, OOM) */
  DHW_ERR_STATE = -4,     /* call order (e.g. forward before all weights are loaded) */
  DHW_ERR_INTERNAL = -5   /* a C++ exception (std::bad_alloc, std::out_of_range, ...) or an internal inconsistency inside the library:
                             caught at the ABI (csrc/abi_guard.h), reported through dhw_last_error; the process and the handle stay
                             alive (the failed call's outputs are undefined) */
} dhw_status;

/* dtype codes for dhw_load */
enum { DHW_F32 = 0, DHW_BF16 = 1, DHW_F16 = 2, DHW_F64 = 3 };

/* compute precision of the denoiser */
enum { DHW_PREC_BF16 = 0,  /* bf16 activations + weights, fp32 accumulate/LN/softmax/state (perf mode) */
       DHW_PREC_F32 = 1 }; /* fp32 everywhere, exact-f32 MFMA (parity mode) */

typedef struct {
  int num_layers;   /* bottleneck EncoderLayers (model.py:66; shipped configs use 2) */
  int c1, c2, c3;   /* 128 / 192 / 256 (model.py:67-69); c1 must be 128 and c3 256; c2 any multiple of 12 up to 192
                       (3 / 6 / 8 attention heads, model.py:88-106): widths below 192 run zero-padded inside the 192-wide kernels */
  int max_B;        /* largest batch a call may pass */
  int max_L;        /* largest stroke length (multiple of 8, model.py:169-175) */
  int max_Lt;       /* largest token count */
  int S;            /* style rows: style_vector is [B,S,1280] (S = 14 in use, 1 in the reference test) */
  int precision;    /* DHW_PREC_* */
} dhw_dims;

/* Create a handle on HIP device `device`. */
int dhw_create(dhw_handle** out, const dhw_dims* dims, int device);

/* Hand over one state_dict tensor (HOST pointer, torch-native layout:
 * Linear.weight [out,in], Conv1d.weight [Cout,Cin,3]).  The library copies,
 * casts and repacks; the caller's buffer is free after return.  Unknown key or
 * wrong shape -> DHW_ERR_KEY (strict, like checkpoint.py:83-87).  Loading a key
 * again replaces it (and invalidates the packed copy until the next finalize). */
int dhw_load(dhw_handle*, const char* key, const void* host_ptr, int dtype,
             const int64_t* shape, int ndim);

/* Check that every key of the state_dict is present (DHW_ERR_KEY names the
 * first missing one), pack for the MFMA kernels and upload.  Called implicitly
 * by dhw_forward / dhw_sample when needed. */
int dhw_finalize(dhw_handle*);

/* Number of state_dict keys the handle expects, and the i-th key/shape. */
int dhw_num_keys(dhw_handle*);
int dhw_key_info(dhw_handle*, int i, const char** key, int64_t shape[3], int* ndim);

/* == DiffusionModel.forward(strokes, text, sigma, style_vector) -> (eps, pen)
 * strokes f32 [B,L,2]; text int64 [B,Lt] (0 = pad); sigma f32 [B];
 * style f32 [B,S,1280]; eps_out f32 [B,L,2]; pen_out f32 [B,L] in (0,1).
 * L % 8 == 0, B <= max_B, L <= max_L, Lt <= max_Lt. */
int dhw_forward(dhw_handle*, const float* strokes, const int64_t* text, const float* sigma,
                const float* style, int B, int L, int Lt,
                float* eps_out, float* pen_out, void* hip_stream);

/* == inference.py:80-96 for a batch.  mode 0 = "new" (default), 1 = "standard".
 * noise: f32 [T+1,B,L,2] in consumption order (noise[0] = x_T, noise[1+k] = the
 * draw of the k-th loop iteration) or NULL to draw N(0,1) on the device from
 * (seed, first_sample + b, iteration, position) — identical for any sharding.
 * out: f32 [B,L,3] = cat(x_0, pen of the LAST denoiser call). */
int dhw_sample(dhw_handle*, const int64_t* text, const float* style, int B, int L, int Lt,
               int T, int mode, const float* noise, uint64_t seed, int64_t first_sample,
               float* out, void* hip_stream);

/* Ragged batches: samples of different stroke lengths in one call.  lens is a HOST pointer to B
 * entries, each a multiple of 8 in [8, L]; L is the padded length (the row stride of every [B,L,..]
 * tensor).  Row b computes exactly what the uniform call computes for sample b alone at L = lens[b]
 * (dhw_sample_ragged: with first_sample + b; external noise: noise[:, b, :lens[b], :]).  Outputs past
 * lens[b] are 0; inputs there (strokes, noise) are ignored, whatever they hold.  With every
 * lens[b] == L the result is bit-identical to dhw_forward / dhw_sample.  The lengths are copied to a
 * library-owned device buffer on hip_stream and read by the kernels at run time, so one captured graph
 * serves every set of lengths of a (B, L, Lt, T, mode).  A bad entry -> DHW_ERR_ARG naming it.
 * Every launch configuration supports lengths except the off-by-default persistent step:
 * dhw_sample_ragged on a handle created with DHW_PERSIST=1 -> DHW_ERR_ARG naming the switch. */
int dhw_forward_ragged(dhw_handle*, const float* strokes, const int64_t* text, const float* sigma,
                       const float* style, int B, int L, int Lt, const int32_t* lens,
                       float* eps_out, float* pen_out, void* hip_stream);
int dhw_sample_ragged(dhw_handle*, const int64_t* text, const float* style, int B, int L, int Lt,
                      const int32_t* lens, int T, int mode, const float* noise, uint64_t seed,
                      int64_t first_sample, float* out, void* hip_stream);

/* Conditioned sampling (replacement conditioning of the reverse process): keep the strokes of chosen rows exactly as given
 * (in-painting, completion), start from an existing line noised part of the way up the schedule (restyling), or both.  The
 * arguments are dhw_sample_ragged's, with lens allowed to be NULL (every row has L strokes), plus
 *    known       device f32 [B,L,3] = (dx, dy, pen), or NULL
 *    keep        device uint8 [B,L], nonzero = keep this row, or NULL (nothing kept)
 *    t_start     in [1, T]
 *    cond_noise  device f32 [T,B,L,2], or NULL.
 * Symbols: beta[i], abar[i] as dhw_schedule gives them; loop iteration k = 0..T-1 handles schedule index i = T-1-k, as in
 * dhw_sample; a_next(i) = abar[i-1] for i > 1, else 1 (the reference's quirk, inference.py:87), used for BOTH modes here.
 * A row (b, p) with p < lens[b] (p < L without lens) is KEPT iff keep && keep[b,p], and SEEDED iff it is kept or t_start < T.
 *    1. Iterations run.  Only k = T - t_start .. T-1 run.  Iteration numbers, noise indexing (noise[1+k]) and generator
 *       keys are those of the full call, so t_start = T runs everything.
 *    2. Start.  z = noise[0], or the device draw with iter = -1, exactly as in dhw_sample.  With i0 = t_start - 1, seeded
 *       rows get x = fadd(fmul(sqrtf(abar[i0]), known_xy), fmul(sqrtf(1 - abar[i0]), z)); the others x = z.  Coefficients
 *       are computed on the host in fp32; the device multiplies and adds with round-to-nearest and no contraction.
 *    3. After the update of iteration k (whichever kernel performs it) every kept row is overwritten with
 *       x = fadd(fmul(sqrtf(a_next), known_xy), fmul(sqrtf(1 - a_next), zc)), zc = cond_noise[k,b,p] when external noise is
 *       used, otherwise the generator's draw for (seed, first_sample + b, p, iter = 2^30 + k): an iteration range disjoint
 *       from everything the sampler draws, so the conditioning stream is independent and as sharding-invariant.  The last
 *       two iterations have a_next = 1: kept rows equal known_xy from there on.
 *    4. Output.  Kept rows of out are `known` bit for bit (dx, dy and pen).  Other valid rows are x_0 and the pen of the
 *       last denoiser call, as in dhw_sample.  Rows past lens[b] are 0.
 *    5. Rows that are not read.  Rows of `known` that are neither seeded nor kept, and all rows past lens[b], are never
 *       read: the kernels branch rather than blend, so NaNs there change nothing.  known == NULL is legal only with
 *       keep == NULL and t_start == T; that call is bit-identical to dhw_sample / dhw_sample_ragged.
 *    6. Noise arguments.  cond_noise must be given iff noise is given and keep is non-NULL; otherwise DHW_ERR_ARG naming
 *       the argument.
 *    7. Persistent step.  A handle created with DHW_PERSIST=1 refuses the call with DHW_ERR_ARG naming the switch.
 * Every argument check runs before the first HIP call.  known, keep and cond_noise are copied to library-owned buffers on
 * hip_stream and read by the kernels at run time: one captured graph serves every mask and every `known` of a
 * (shape, t_start, keep given or not, cond_noise given or not). */
int dhw_sample_cond(dhw_handle*, const int64_t* text, const float* style, int B, int L, int Lt,
                    const int32_t* lens, int T, int mode, const float* noise, uint64_t seed,
                    int64_t first_sample, const float* known, const uint8_t* keep, int t_start,
                    const float* cond_noise, float* out, void* hip_stream);

/* Scoring: the denoising objective (the reference's training loss, loss.py:29-37) of strokes that already exist, at chosen
 * noise levels — how well a line fits a text and a hand under the model.  Nothing is sampled.
 *    strokes  device f32 [B,L,3] = (dx, dy, pen)
 *    lens     HOST int32 [B] or NULL (every row has L strokes); the rules for lens are dhw_forward_ragged's
 *    levels   HOST int32 [K]: schedule indices, 0 <= levels[k] < T; duplicates allowed, any order; 1 <= K <= T
 *    noise    device f32 [K,B,L,2], or NULL
 *    out      device f32 [K,B,2]
 * Symbols: beta[i], abar[i] as dhw_schedule(T) gives them; n = lens[b] (L without lens); i = levels[k].
 *    1. Noise.  z[k,b,p] = noise[k,b,p,:] when noise is given; otherwise the generator's draw for (seed, first_sample + b,
 *       p, iter = 2^29 + i): an iteration range disjoint from the sampler's (-1 .. T-1) and from the conditioning
 *       stream's (2^30 + k).  The draw is keyed by the schedule index i, not by k: the score at a level depends neither on
 *       which other levels are asked for nor on how the batch is sharded.
 *    2. Perturbation.  x_t = fadd(fmul(sqrtf(abar[i]), x0), fmul(sqrtf(1 - abar[i]), z)), x0 = strokes[..., :2].  The
 *       coefficients are computed on the host in fp32; the device rounds each product and the sum, no contraction.
 *    3. Denoiser.  (eps_hat, pen_hat) = dhw_forward_ragged(x_t, text, sigma = sqrtf(abar[i]) for every row, style, lens):
 *       the same launches and the same precision as that entry, on every handle (DHW_PERSIST=1 included).
 *    4. Outputs, both means over the valid rows of sample b only:
 *          out[k,b,0] = (1/n) sum_{p<n} ((z0 - e0)^2 + (z1 - e1)^2)
 *          out[k,b,1] = abar[i] * (1/n) sum_{p<n} -( t * max(logf(q), -100) + (1 - t) * max(logf(1 - q), -100) ),
 *       q = pen_hat[p], t = clamp(pen[p], 1e-7, 1 - 1e-7): torch's binary_cross_entropy after the clamp of loss.py:31.
 *       Without lens, the mean over b of out[k,:,0] + out[k,:,1] is the reference's loss_fn(...)[0] at alphas = abar[i].
 *    5. Rows that are not read.  Rows of strokes and noise at or past lens[b] are never read: NaNs there change nothing.
 *    6. Determinism.  Fixed reduction order, no float atomics: the result is bit-deterministic, and out[:, b] of a batch
 *       equals sample b scored alone at L = lens[b] with first_sample + b, bit for bit.
 *    7. Argument checks.  Every check runs before the first HIP call and returns DHW_ERR_ARG naming the argument: the
 *       forward entry's limits (B, L, Lt, lens), 1 <= T <= 2^29, 1 <= K <= T, 0 <= levels[k] < T, non-NULL strokes / text /
 *       style / levels / out, out and noise 8-byte aligned.
 * The K levels run as K denoiser calls over B rows on hip_stream, launched eagerly.  The call reads strokes, text, style and
 * noise in place (they must stay valid until the stream has run it), stages x_t, z and the denoiser's outputs in buffers the
 * handle allocates at its first score call, and neither alters nor invalidates anything dhw_sample* has cached. */
int dhw_score(dhw_handle*, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt,
              const int32_t* lens, int T, const int32_t* levels, int K, const float* noise, uint64_t seed,
              int64_t first_sample, float* out, void* hip_stream);

/* Attention maps: which text token each stroke row attends to.  Every EncoderLayer cross-attends its stroke rows to the text
 * tokens (model.py:46); the original network returned that map as its third output.  dhw_attention is one denoiser call that
 * also writes the map of one layer.  `layer` is numbered as in dhw_debug_attention_time:
 *    layer 0 = enc3            H = 3 heads, Lq = L/2 rows
 *    layer 1 = enc5            H = 4,       Lq = L/4
 *    layer 2 + i = att_layers.i  H = 6,     Lq = L/8
 * dhw_attention_shape gives (H, Lq) for a layer and a length; it needs no device, and with a NULL handle it answers for any
 * model (only a handle's own limits, its layer count and max_L, are then not checked).
 *    strokes, text, sigma, style, eps_out, pen_out   as dhw_forward (device)
 *    lens        HOST int32 [B] or NULL (every row has L strokes); the rules for lens are dhw_forward_ragged's
 *    probs_out   device f32 [B,H,Lq,Lt] or NULL
 *    mean_out    device f32 [B,Lq,Lt] or NULL
 *    token_out   device int32 [B,Lq] or NULL
 *    1. Outputs of the forward.  eps_out and pen_out are exactly what dhw_forward (lens == NULL) or dhw_forward_ragged writes
 *       for the same arguments on the same handle, bit for bit: the call is that forward plus what follows.
 *    2. Probabilities.  P[b,h,q,k] = softmax_k(Q[b,q,h,:] . K[b,k,h,:] / 8 + (text[b,k] == 0) * (-1e9)), all in fp32, the
 *       dot product a k-ordered fmaf chain over the 64 channels of the head.  Q = Wq(x + PE) of the layer's `mha`, evaluated
 *       on the layer input the forward left in the workspace; K is that call's text keys of the layer; both in the handle's
 *       element type (heads narrower than 64 are zero-padded to 64 and their scale is folded into Wq, so the divisor is
 *       always 8).  On a bf16 handle this is the map of the stored bf16 operands; it is not promised to be what the fused
 *       kernels hold internally.  A masked key gets exactly 0.0 whenever the prompt has a non-pad token; an all-pad prompt
 *       gets 1/Lt everywhere, as the reference does.
 *    3. Mean and token.  mean[b,q,k] = (((P[b,0] + P[b,1]) + P[b,2]) + ...) * (1/H), in head order, 1/H rounded to fp32;
 *       token[b,q] = the smallest k at which mean[b,q,:] is largest.  NaN compares larger than nothing: a row of mean that
 *       is NaN throughout (non-finite weights or inputs) gets token 0, so a valid row's token always lies in [0, Lt).
 *    4. Ragged rows.  With n = lens[b] >> shift (shift = 1, 2, 3 as Lq = L/2, L/4, L/8): rows q >= n of probs and mean are 0
 *       and token is -1.  Nothing of strokes past lens[b] is read.  Row b equals its alone run at L = lens[b], bit for bit
 *       (every sum's order depends on the row alone); with every lens[b] == L the call equals the uniform one.
 *    5. Argument checks.  Each answers DHW_ERR_ARG, naming the argument and dhw_attention, before dhw_finalize, the first
 *       thing that can touch HIP: null handle, strokes, text, sigma, style, eps_out or pen_out; the forward entry's limits
 *       (B, L, Lt, lens); 0 <= layer < 2 + num_layers; at least one of probs_out / mean_out / token_out non-NULL; probs_out
 *       and mean_out 16-byte aligned; Lt <= 168 (what the kernel's LDS tile holds without a raised limit).
 *    6. Side effects.  Like dhw_score the call launches eagerly on hip_stream — the forward's launches, one GEMM for Q into
 *       a workspace buffer, one map kernel — and works on a handle created with DHW_PERSIST=1.  It touches neither the
 *       sampler's staging buffers and graph cache nor its generator state. */
int dhw_attention_shape(dhw_handle*, int layer, int L, int* heads_out, int* Lq_out);
int dhw_attention(dhw_handle*, const float* strokes, const int64_t* text, const float* sigma, const float* style,
                  int B, int L, int Lt, const int32_t* lens, int layer,
                  float* probs_out, float* mean_out, int32_t* token_out,
                  float* eps_out, float* pen_out, void* hip_stream);

/* Deterministic (DDIM, eta = 0) sampling over a sub-sequence of the schedule, and its inversion: the latent an existing line
 * came from.  The denoiser is conditioned on the continuous sigma = sqrt(abar), so it can be asked at any subset of the T
 * levels; a deterministic step draws no noise, so a line is a function of its start latent alone.
 * Symbols: beta[i], abar[i] as dhw_schedule(T) gives them.  levels is a HOST int32 [S] of schedule indices, STRICTLY
 * DECREASING, 0 <= levels[j] < T, 1 <= S <= T.  a_j = abar[levels[j]] for j < S and a_S = 1, the clean end.
 * Coefficients, computed on the host in fp32: A_j = sqrtf(a_j), B_j = sqrtf(1.0f - a_j); A_S = 1, B_S = 0.
 * The update, per stroke row and per coordinate:
 *    U(base, e; c0, c1, c2, c3) = fadd(fmul(c2, fdiv(fsub(base, fmul(c1, e)), c0)), fmul(c3, e)),
 * every operation rounded to nearest (the division correctly rounded), nothing contracted: the x0 estimate from (base, e) at
 * level (c0, c1), moved to level (c2, c3) along the same e.
 *
 * dhw_ddim_sample
 *    text, style   as dhw_forward (device);  lens  HOST int32 [B] or NULL, the rules of dhw_forward_ragged
 *    latent        device f32 [B,L,2], or NULL;  latent_out  device f32 [B,L,2], or NULL;  out  device f32 [B,L,3]
 *    1. Start.  x(0) = latent when it is given; otherwise the generator's draw for (seed, first_sample + b, p, iter = -1),
 *       the x_T dhw_sample draws.  latent_out receives x(0).
 *    2. Steps j = 0..S-1.  (e, q) = the forward of x(j) with sigma = A_j for every row: the same launches and the same
 *       precision as dhw_forward_ragged (dhw_forward when lens == NULL).  x(j+1) = U(x(j), e; A_j, B_j, A_{j+1}, B_{j+1}).
 *    3. Output.  out[b,p] = (x(S)[b,p], q of the last call) for p < lens[b].  Rows at or past lens[b] of out and latent_out
 *       are 0; rows of latent there are never read.
 *
 * dhw_ddim_invert
 *    strokes  device f32 [B,L,3] (the pen column is not read);  latent_out  device f32 [B,L,2];  1 <= iters <= 8
 *    1. Start.  y(S) = strokes[..., :2].
 *    2. Steps j = S-1 down to 0.  w = y(j+1); iters times: (e, _) = the forward of w at sigma = A_j, then
 *       w = U(y(j+1), e; A_{j+1}, B_{j+1}, A_j, B_j); then y(j) = w.  iters = 1 is the usual DDIM inversion; more iterations
 *       are the fixed-point refinement of the same equation, whose fixed point is, in exact arithmetic, the exact inverse of
 *       step j of the sampler.
 *    3. Output.  latent_out = y(0), rows at or past lens[b] 0; rows of strokes there are never read.
 *    4. The call makes S * iters denoiser calls.
 *
 * dhw_ddim_update
 *    The one update kernel on given device arrays, so that it can be pinned bit for bit on its own: out[r] = U(base[r], eps[r];
 *    c0, c1, c2, c3) for the rows r = b*L + p with p < lens[b], 0 for the others, which are not read.  base, eps, out device
 *    f32 [B,L,2] (out may be base); lens DEVICE int32 [B] or NULL, any 0 <= n (n >= L: every row).  No handle: errors are
 *    read through dhw_last_error(NULL).  B, L >= 1, B * L < 2^31.
 *
 * Rules for all three entries.
 *    Arguments.  Every check runs before the first HIP call and returns DHW_ERR_ARG naming the argument: the forward entry's
 *       limits (B, L, Lt, lens); 1 <= T <= 2^29; 1 <= S <= T; every levels[j] in range and the array strictly decreasing;
 *       iters in [1, 8]; required pointers non-NULL; latent, latent_out, base, eps and dhw_ddim_update's out 8-byte aligned.
 *    Determinism.  No atomics, no reductions: the result is bit-deterministic; row b of a batch equals sample b run alone at
 *       L = lens[b] with first_sample + b, bit for bit; with every lens[b] == L the result equals the call with lens == NULL.
 *    Side effects, as for dhw_score.  Launches are eager on hip_stream.  The state x, the iterate w, the denoiser's outputs
 *       and sigma live in buffers the handle allocates, at its capacity, at its first ddim call.  text, style, latent and
 *       strokes are read in place (they must stay valid until the stream has run the call).  Nothing of the sampler's is
 *       touched: not its graph cache, its generator state, its staging buffers or its step plans.  The entries work on a
 *       handle created with DHW_PERSIST=1. */
int dhw_ddim_sample(dhw_handle*, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens,
                    int T, const int32_t* levels, int S, const float* latent, uint64_t seed, int64_t first_sample,
                    float* latent_out, float* out, void* hip_stream);
int dhw_ddim_invert(dhw_handle*, const float* strokes, const int64_t* text, const float* style, int B, int L, int Lt,
                    const int32_t* lens, int T, const int32_t* levels, int S, int iters, float* latent_out,
                    void* hip_stream);
int dhw_ddim_update(const float* base, const float* eps, const int32_t* lens, int B, int L,
                    float c0, float c1, float c2, float c3, float* out, void* hip_stream);

/* Classifier-free guidance: sampling that extrapolates from the denoiser's answer under a GUIDANCE condition (by default the
 * null condition: the prompt [1, 0, 0, ...] = the end token then padding, and an all-zero style; training hides both with
 * dhw_train_cond_drop) towards its answer under the real one.  Scale 1 is the ordinary sample, larger scales trade diversity for
 * legibility, scale 0 is the guidance condition's own sample.
 *
 * The guided noise estimate of stroke row (b, p), per coordinate, with e_c the denoiser's eps under the real condition, e_u under
 * the guidance condition and w = scale[b]:
 *    e = fadd(e_c, fmul(fsub(w, 1), fsub(e_c, e_u)))     for w != 0;        e = e_u     for w == 0.
 * Every operation is rounded to nearest, nothing is contracted.  At w = 1 the product is a zero and e has e_c's value (a -0 may
 * become +0).  The arithmetic alone gives e_c - fl(e_c - e_u) at w = 0, which is e_u only where that difference is exact; w = 0 is
 * therefore a select, so that scale 0 IS the sample under the guidance condition.  The pen probability is the conditional row's.
 *
 * One forward per step.  text2 int64 [2B,Lt] and style2 f32 [2B,S,1280] (device): rows [0, B) hold the real condition, rows
 * [B, 2B) the guidance condition of rows [0, B).  The state holds x twice; each step is one forward of the 2B rows (the launches
 * and the precision of dhw_forward_ragged, dhw_forward when lens == NULL) and one step kernel that reads x[b], e[b] and e[b+B] and
 * writes the new row to x[b] and x[b+B].  lens: HOST int32 [B] or NULL, the rules of dhw_forward_ragged; it applies to both halves.
 * scale: HOST f32 [B], every entry finite and in [0, 64].  2B <= the handle's max_B.
 *
 * dhw_guided_ddim_sample
 *    T, levels, S, latent, seed, first_sample, latent_out, out: as dhw_ddim_sample.  x(0) as there; steps j = 0..S-1:
 *    x(j+1) = U(x(j), e; A_j, B_j, A_{j+1}, B_{j+1}) with dhw_ddim_sample's U, coefficient table and levels.  out[b,p] =
 *    (x(S)[b,p], q_c of the last call) for p < lens[b]; rows at or past lens[b] of out and latent_out are 0.
 *
 * dhw_guided_sample
 *    T, mode, noise, seed, first_sample, out: as dhw_sample.  x_T = noise[0], or the generator's draw for (seed, first_sample + b, p,
 *    iter = -1).  Iteration k = 0..T-1 at schedule index i = T-1-k, sigma = sqrtf(abar_i) for every row, with the coefficients
 *    dhw_sample computes on the host in fp32 and z = noise[1+k][b,p] (noise f32 [T+1,B,L,2], device) or the generator's draw for
 *    (seed, first_sample + b, p, k) — the keys dhw_sample uses:
 *       mode 0 ("new"):       x = fadd(fdiv(fsub(x, fmul(k0, e)), k1), fmul(z, k2))
 *       mode 1 ("standard"):  x = fmul(k1, fsub(x, fdiv(fmul(k3, e), k0))), then for i != 0 x = fadd(x, fmul(k2, z))
 *    one rounding per operation, dhw_sample's own order.  out[b,p] = (x, q_c of the last call), 0 at and past lens[b].
 *
 * dhw_guide_update
 *    The one step kernel on given device arrays, so that it can be pinned bit for bit on its own.  kind 0: U(base, e; c0..c3); 1:
 *    the "new" step with (k0, k1, k2) = (c0, c1, c2); 2: the "standard" step with (k0, k1, k2, k3) = (c0, c1, c2, c3).  base: device
 *    f32, rows [0, B L) x 2 are read; eps2 f32 [2B,L,2]; pen f32, rows [0, B L) (read only with out3; NULL without it); lens DEVICE
 *    int32 [B] or NULL, any 0 <= n (n >= L: every row); scale DEVICE f32 [B] (not range-checked: it is device memory); z f32 [B,L,2]
 *    or NULL: the noise term is added iff z is given (kind 0 takes none).  out f32 [2B,L,2] or NULL: row r = b L + p and row r + B L
 *    both receive the new value (out may be base); out3 f32 [B,L,3] or NULL = (new value, pen).  Rows at or past lens[b] are
 *    written as 0 and not read.  No handle: errors are read through dhw_last_error(NULL).  B, L >= 1, 2 B L < 2^31.
 *
 * Rules for the entries.
 *    Arguments.  Every check runs before the first HIP call and returns DHW_ERR_ARG naming the argument: required pointers
 *       non-NULL; the forward entry's limits (B, L, Lt, lens); the level checks of dhw_ddim_sample, or 1 <= T <= 2^29 and mode 0 / 1;
 *       every scale finite and within [0, 64]; 2B <= max_B (both numbers are in the message); 2 B L < 2^31; latent, latent_out,
 *       noise, base, eps2, z and dhw_guide_update's out 8-byte aligned.
 *    Determinism.  No atomics, no reductions: the result is bit-deterministic; row b equals sample b run alone at L = lens[b]
 *       with first_sample + b and scale[b]; a row's result does not depend on the other rows' scales.
 *    Side effects, as for dhw_ddim_sample.  Launches are eager on hip_stream.  The state lives in the ddim entries' scratch set
 *       (x, eps, pen, sigma) used at 2B rows; the scales are copied to a [max_B] device array the handle allocates at its first guided
 *       call and never moves.  Nothing of the sampler's is touched: not its graph cache, its generator state, its staging
 *       buffers, its step plans or its text-plane tag.  The entries work on a handle created with DHW_PERSIST=1. */
int dhw_guided_ddim_sample(dhw_handle*, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens,
                           int T, const int32_t* levels, int S, const float* scale, const float* latent, uint64_t seed,
                           int64_t first_sample, float* out, float* latent_out, void* hip_stream);
int dhw_guided_sample(dhw_handle*, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens, int T,
                      int mode, const float* scale, const float* noise, uint64_t seed, int64_t first_sample, float* out,
                      void* hip_stream);
int dhw_guide_update(int kind, const float* base, const float* eps2, const float* pen, const int32_t* lens, const float* scale,
                     const float* z, int B, int L, float c0, float c1, float c2, float c3, float* out, float* out3,
                     void* hip_stream);

/* Second-order multistep sampling (DPM-Solver++ 2M) over the levels of dhw_ddim_sample: the same number of denoiser calls, each
 * step between the first and the last also using the x0 estimate the previous step left behind.
 *
 * Setup.  levels, a_j, A_j = sqrtf(a_j), B_j = sqrtf(1 - a_j) and (A_S, B_S) = (1, 0) are exactly dhw_ddim_sample's.  order is 1 or
 * 2.  Step j (0 <= j < S) moves the state from level j to level j + 1 using (e_j, q_j), the forward of x_j at sigma = A_j (guided:
 * e_j is dhw_guided_ddim_sample's combination of the two halves).  Every step first computes, with the first three operations of U,
 *    x0_j = fdiv(fsub(x_j, fmul(B_j, e_j)), A_j).
 *
 * First-order steps: j = 0, j = S - 1 (it goes to B = 0, where log-SNR is infinite), and every step when order = 1.
 *    x_{j+1} = U(x_j, e_j; A_j, B_j, A_{j+1}, B_{j+1}): the bits of dhw_ddim_update.  Then hist <- x0_j.
 *
 * Second-order steps: 0 < j < S - 1 when order = 2.  On the HOST, in double from the fp32 A, B of the table, each result rounded
 * once to fp32:
 *    lambda_j = log(A_j / B_j),  h = lambda_{j+1} - lambda_j,  r = (lambda_j - lambda_{j-1}) / h,
 *    k1 = 1 / (2 r),  k0 = 1 + k1,  c4 = B_{j+1} / B_j,  c5 = -A_{j+1} expm1(-h).
 * On the device, nine fp32 operations per coordinate, each rounded to nearest, nothing contracted:
 *    m = B_j e;  d = x - m;  x0 = d / A_j;  p = k0 x0;  q = k1 hist;  D = p - q;  s = c4 x;  n = c5 D;  x' = s + n.
 * Then hist <- x0.  (In exact arithmetic: x' = (B_{j+1}/B_j) x + A_{j+1} (1 - e^{-h}) ((1 + 1/(2r)) x0_j - (1/(2r)) x0_{j-1}).)
 *
 * Edge cases.  A table whose h or r is not finite and positive (levels whose fp32 a_j coincide or reach 1) is refused with
 * DHW_ERR_ARG before any HIP call.  Step 0 never reads hist.  Rows at or past lens[b] are never read, in base, eps or hist; they are
 * written as 0 in out and hist.  With S <= 2 every step is first order: order = 2 then returns dhw_ddim_sample's bits.
 *
 * dhw_dpm_coefs
 *    The table the library uses, on the host, no handle: out is a HOST f32 [S][9] = (kind, c0, c1, c2, c3, k0, k1, c4, c5) per step:
 *    kind 1 (first order) or 2 (second order); (c0, c1, c2, c3) = (A_j, B_j, A_{j+1}, B_{j+1}) in every row; (k0, k1, c4, c5) as
 *    above in a second-order row and 0 in a first-order one.  T, levels, S as dhw_ddim_sample; errors through dhw_last_error(NULL).
 *
 * dhw_dpm_update
 *    The one step kernel on given device arrays, so that it can be pinned bit for bit on its own.  coef: HOST f32 [9], a row of
 *    dhw_dpm_coefs' layout (coef[0] must be 1 or 2).  base, eps, out device f32 [B,L,2] (out may be base); hist device f32 [B,L,2],
 *    read (kind 2 only) and written in place; lens DEVICE int32 [B] or NULL, any 0 <= n.  scale DEVICE f32 [B] or NULL: with it the
 *    step is the guided one: eps is [2B,L,2], e = the combination of eps[r] and eps[r + B L] at scale[b], out is [2B,L,2] and rows r
 *    and r + B L both receive x'; hist stays [B,L,2].  out3 f32 [B,L,3] or NULL = (x', pen[r]); pen f32 [B,L] is read with out3 only.
 *    One of out / out3 is needed.  base, eps, hist, out 8-byte aligned.  No handle: errors through dhw_last_error(NULL).  B, L >= 1,
 *    B L (2 B L with a scale) < 2^31.
 *
 * dhw_dpm_sample, dhw_guided_dpm_sample
 *    The argument lists, the start, the output, the checks, the determinism and the side effects of dhw_ddim_sample and
 *    dhw_guided_ddim_sample, plus order (1 or 2, checked behind the levels; then the table's h and r).  Every check answers before
 *    dhw_finalize.  hist is a fifth buffer [max_B max_L, 2] of the eager entries' scratch set, allocated at the first such call and
 *    never moved; every call writes it at step 0 before any step reads it, so nothing carries over from call to call.  The
 *    coefficients travel to the kernel by value; no graph is used.  Nothing of the sampler's is touched.  The entries work on a
 *    handle created with DHW_PERSIST=1. */
int dhw_dpm_coefs(int T, const int32_t* levels, int S, int order, float* out);
int dhw_dpm_update(const float* base, const float* eps, const float* pen, const int32_t* lens, const float* scale, float* hist,
                   int B, int L, const float* coef, float* out, float* out3, void* hip_stream);
int dhw_dpm_sample(dhw_handle*, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens,
                   int T, const int32_t* levels, int S, int order, const float* latent, uint64_t seed, int64_t first_sample,
                   float* latent_out, float* out, void* hip_stream);
int dhw_guided_dpm_sample(dhw_handle*, const int64_t* text2, const float* style2, int B, int L, int Lt, const int32_t* lens,
                          int T, const int32_t* levels, int S, int order, const float* scale, const float* latent, uint64_t seed,
                          int64_t first_sample, float* out, float* latent_out, void* hip_stream);

/* Stroke rasteriser: sampled strokes -> grey-level line images in the layout dhw_style_forward consumes (ink
 * left-aligned, white to the right).  No handle: errors are read through dhw_last_error(NULL).  The call allocates
 * nothing, synchronises nothing and can be captured into a graph.  All argument checks run before the first HIP call
 * (DHW_ERR_ARG names the argument): B >= 1, 1 <= L <= 4096, H >= 8, W >= 8 and W % 4 == 0, 0.5 <= line_width <= 16
 * with 2m < H and 2m < W (m below), non-NULL strokes / img_out / workspace (both 16-byte aligned),
 * workspace_bytes >= dhw_render_workspace_bytes(B, L) (0 for a B or L outside the ranges above).
 *
 * The picture of row b, with n = lens[b] (L when lens is NULL) and (dx, dy, pen)[i] its strokes for i < n (rows at or
 * past n are never read, whatever they hold):
 *    1. pos[i] = sum_{j<=i} (dx_j, dy_j).
 *    2. lift[i] = (rintf(pen[i]) != 0): round-half-to-even, 0.5 is not a lift.
 *    3. last = the largest i with lift[i].
 *    4. Segment i runs from pos[i-1] to pos[i]; it is drawn iff 1 <= i < last and !lift[i]  (nothing after the last lift
 *       is drawn, a row without a lift draws nothing: the consecutive point pairs inside the polylines of the
 *       reference's show_strokes).
 *    5. (xmin, xmax, ymin, ymax) = the box of the endpoints of drawn segments.  No drawn segment: the image is all 255
 *       and widths_out[b] = 0.
 *    6. m = line_width/2 + 1.
 *    7. s = (H - 2m)/(ymax - ymin); if (xmax - xmin) s > W - 2m then s = (W - 2m)/(xmax - xmin).  Both extents 0: s = 1.
 *       Only the height 0: s from the width rule, but never above H - 2m.
 *    8. px = m + (x - xmin) s.
 *    9. py = m + voff + (ymax - y) s, voff = (H - 2m - (ymax - ymin) s)/2  (the stroke y axis points up, image rows go
 *       down; the ink is centred vertically when the width limits the scale).
 *   10. Pixel (r, c) has its centre at (c + 0.5, r + 0.5).
 *   11. d = the smallest Euclidean distance from that centre to a drawn segment (a zero-length segment is a point).
 *   12. value = 255 (1 - clamp(line_width/2 + 0.5 - d, 0, 1)).
 *   13. widths_out[b] = min(W, ceil((xmax - xmin) s + 2m)).
 * The minimum is exact and commutative and no float atomics are used: the image is bit-deterministic, and row b of a
 * batch equals the same strokes rendered alone at L = lens[b], bit for bit. */
size_t dhw_render_workspace_bytes(int B, int L);
int dhw_render(const float* strokes,      /* device f32 [B,L,3]                        */
               const int32_t* lens,       /* DEVICE int32 [B] or NULL, any 1 <= n <= L (unlike the sampler's host lens:
                                             the call chains behind dhw_sample_ragged without a host read) */
               int B, int L, int H, int W, float line_width,
               float* img_out,            /* device f32 [B,1,H,W], 0..255              */
               int32_t* widths_out,       /* device [B] or NULL                        */
               void* workspace, size_t workspace_bytes, void* hip_stream);

/* Page compositor: N lines -> P page images, every line drawn at ONE scale in a slot of its own, ink that reaches into a
 * neighbouring slot composed by min.  (dhw_render scales each line to fill its own image: stacked, those do not make a
 * page.)  No handle: errors are read through dhw_last_error(NULL).  The call allocates nothing, synchronises nothing and
 * can be captured into a graph.  All argument checks run before the first HIP call (DHW_ERR_ARG names the argument):
 * 1 <= N <= 4096, 1 <= L <= 4096, P >= 1, H >= 8, W >= 8 and W % 4 == 0, P H W < 2^31 (and within the launch grid:
 * P ceil(W/32) < 2^24, ceil(H/96) <= 65535), lines_per_page >= 1, pitch > 0, margin_left >= 0, margin_top >= 0,
 * W - 2 margin_left > 0, 0.5 <= line_width <= 16, scale >= 0, every float finite, non-NULL strokes / pages / scale_out /
 * boxes_out / workspace, pages and workspace 16-byte aligned, workspace_bytes >= dhw_page_workspace_bytes(N, L) (0 for an
 * N or L outside the ranges above).
 *
 * Line n, with lens[n] (L when lens is NULL) strokes and slot[n] = slots[n] (n when slots is NULL):
 *    1.-5. as dhw_render, unchanged: pos = the prefix sums, lift[i] = (rintf(pen[i]) != 0), last = the largest i with a
 *       lift, segment i is drawn iff 1 <= i < last and !lift[i] (nothing after the last lift is drawn), and
 *       (xmin, xmax, ymin, ymax)_n = the box of the endpoints of drawn segments.
 *    6. A line without a drawn segment, and a line whose slot lies outside [0, P lines_per_page), draws nothing and takes
 *       no part in the scale.
 *    7. ex_n = xmax_n - xmin_n, ey_n = ymax_n - ymin_n.  s_n = the smaller of pitch / ey_n (when ey_n > 0) and
 *       (W - 2 margin_left) / ex_n (when ex_n > 0); both extents 0: s_n = +inf.  Each quotient is one fp32 division,
 *       W - 2 margin_left is formed in fp32.
 *    8. s = scale when scale > 0, else (automatic) the minimum of s_n over the lines that take part, or 1 if none is
 *       finite.  min is exact and commutative: s does not depend on the order of the lines, no float atomics are used.
 *    9. Line n goes to page slot[n] / lines_per_page;  top_n = margin_top + (slot[n] % lines_per_page) pitch.
 *   10. px = margin_left + (x - xmin_n) s.
 *   11. py = top_n + (pitch - ey_n s)/2 + (ymax_n - y) s  (the stroke y axis points up, page rows go down; the ink box is
 *       centred in its slot).
 *   12. Pixel (r, c) of a page has its centre at (c + 0.5, r + 0.5); d = the smallest Euclidean distance from that centre
 *       to a drawn segment of ANY line of that page (a zero-length segment is a point); value = 255 (1 - clamp(
 *       line_width/2 + 0.5 - d, 0, 1)).  Ink outside the page is clipped.  With an explicit scale lines may overlap their
 *       neighbours: that is allowed and composes by min.
 *   13. scale_out[0] = s.  boxes_out[n] = (margin_left, top_n + (pitch - ey_n s)/2, margin_left + ex_n s, that top +
 *       ey_n s): left, top, right, bottom of the line's ink box in page pixels; all four 0 for a line that draws nothing.
 * The pages are bit-deterministic, independent of the order of the lines, and equal to the element-wise minimum of the
 * pages of each line drawn alone at scale s. */
size_t dhw_page_workspace_bytes(int N, int L);
int dhw_page(const float* strokes,      /* device f32 [N,L,3]                                             */
             const int32_t* lens,       /* DEVICE int32 [N] or NULL, any 1 <= n <= L                      */
             const int32_t* slots,      /* DEVICE int32 [N] or NULL (slot[n] = n)                         */
             int N, int L, int P, int H, int W, int lines_per_page,
             float margin_left, float margin_top, float pitch,      /* page pixels                        */
             float line_width, float scale,                         /* scale 0: automatic                 */
             float* pages,              /* device f32 [P,1,H,W], 0..255                                   */
             float* scale_out,          /* device f32 [1]                                                 */
             float* boxes_out,          /* device f32 [N,4]                                               */
             void* workspace, size_t workspace_bytes, void* hip_stream);

/* Stroke paths: the vector twin of dhw_page.  N lines -> the pen-down polylines of every line in page pixels, at dhw_page's
 * ONE shared scale and in dhw_page's slots, smoothed, thinned, with a tangent per point (a cubic Bezier segment from point k
 * to k + 1 has the control points P_k + t_k and P_k+1 - t_k+1: the Catmull-Rom spline through the kept points).  No handle:
 * errors are read through dhw_last_error(NULL).  The call allocates nothing, synchronises nothing and can be captured into a
 * graph.  All argument checks run before the first HIP call (DHW_ERR_ARG names the argument): N, L, P, H, W, lines_per_page,
 * margin_left, margin_top, pitch, scale and strokes by dhw_page's rules (there is no line_width); 0 <= smooth <= 8,
 * 0 <= rounds <= 8, tol finite and >= 0; non-NULL points_out / index_out / counts_out / scale_out / boxes_out / workspace;
 * points_out and workspace 16-byte aligned, every other pointer 4-byte aligned; workspace_bytes >=
 * dhw_paths_workspace_bytes(N, L) (0 for an N or L outside the ranges).
 *
 * Line n, with lens[n] (L when lens is NULL) strokes and slot[n] = slots[n] (n when slots is NULL):
 *    1. Rules 1.-5. of dhw_render, unchanged: pos = the prefix sums (in the line rasteriser's summation order: the positions
 *       have the raster's bits), lift, last, segment i is drawn iff 1 <= i < last and !lift[i], (xmin, xmax, ymin, ymax)_n =
 *       the box of the endpoints of drawn segments.  A device-side lens entry outside [1, L] is clamped to [0, L].
 *    2. Rules 6.-9. of dhw_page, unchanged: which lines take part, ex_n, ey_n and s_n, the shared s (scale when scale > 0),
 *       the page slot[n] / lines_per_page and top_n = margin_top + (slot[n] % lines_per_page) pitch.
 *    3. Position i (0 <= i < lens) is a path point iff segment i or segment i + 1 is drawn (segment 0 and segment lens never
 *       are).  It starts a polyline iff segment i is not drawn and ends one iff segment i + 1 is not.  Polylines are numbered
 *       0, 1, ... in stroke order; each has at least 2 points; a position belongs to at most one.
 *    4. Placement, fp32: x = margin_left + (pos.x - xmin_n) s;  oy = top_n + (pitch - ey_n s) 0.5;  y = oy + (ymax_n - pos.y) s.
 *       Here and below every difference, product, sum and quotient is one fp32 operation in the order written; none is fused.
 *    5. Smoothing, `smooth` times: every point that neither starts nor ends a polyline becomes (p[i-1] + p[i+1]) 0.25 +
 *       p[i] 0.5 per coordinate, all from the values before the pass.  End points never move.
 *    6. Thinning, `rounds` times, tol2 = tol tol.  At the start of a round the rank of a kept point is the number of kept
 *       points of its polyline before it.  A kept point P is a candidate iff its rank is odd and it does not end its polyline;
 *       A = its previous and B = its next kept neighbour (both of even rank: they survive the round).  With ab = B - A,
 *       ap = P - A and len2 = ab.x ab.x + ab.y ab.y:  d2 = ap.x ap.x + ap.y ap.y if len2 == 0, else t = min(max((ap.x ab.x +
 *       ap.y ab.y) / len2, 0), 1), e = ap - t ab, d2 = e.x e.x + e.y e.y.  P is removed iff d2 <= tol2.  All decisions of a
 *       round use the state at its start.  What this bounds: a point removed in a round lies within tol of the segment
 *       between its neighbours OF THAT ROUND.  Later rounds may remove those neighbours, so after r rounds a removed point
 *       may lie further than tol from the final path.  This is not Ramer-Douglas-Peucker and no global error bound is
 *       claimed; rounds = 0 keeps every point.
 *    7. Tangent of a kept point: t = (next - prev) / 6.0f per coordinate, next / prev = its kept neighbours in the same
 *       polyline, the point itself where there is none.
 *    8. Outputs, compacted in stroke order: row k of points_out[n] = (x, y, tx, ty) of the k-th kept point, row k of
 *       index_out[n] = (i, polyline number).  Rows at or past the count hold 0 in points_out and (-1, -1) in index_out.
 *       counts_out[n] = (kept points, polylines); (0, 0) for a line that takes no part.
 *    9. scale_out[0] = s.  boxes_out[n] = (margin_left, oy, margin_left + ex_n s, oy + ey_n s) with oy of rule 4, each
 *       operation on its own (dhw_page may fuse them: the two boxes can differ in the last bit); zeros for a line that takes
 *       no part.
 *   10. No atomics, one writer per output element: the same call gives the same bits; line n inside any batch has the bits
 *       of line n alone (N = 1, the same slot, scale = the batch's s); the result does not depend on the order of the lines. */
size_t dhw_paths_workspace_bytes(int N, int L);
int dhw_paths(const float* strokes,      /* device f32 [N,L,3]                                             */
              const int32_t* lens,       /* DEVICE int32 [N] or NULL, any 1 <= n <= L                      */
              const int32_t* slots,      /* DEVICE int32 [N] or NULL (slot[n] = n)                         */
              int N, int L, int P, int H, int W, int lines_per_page,
              float margin_left, float margin_top, float pitch,      /* page pixels                        */
              float scale,                                           /* 0: automatic                       */
              int smooth, float tol, int rounds,                     /* tol in page pixels                 */
              float* points_out,         /* device f32 [N,L,4] = (x, y, tx, ty), page pixels               */
              int32_t* index_out,        /* device i32 [N,L,2] = (stroke row i, polyline number)           */
              int32_t* counts_out,       /* device i32 [N,2]   = (kept points, polylines)                  */
              float* scale_out,          /* device f32 [1]                                                 */
              float* boxes_out,          /* device f32 [N,4]                                               */
              void* workspace, size_t workspace_bytes, void* hip_stream);

/* Page ground truth: where every group of stroke rows (a word, a character) sits on the pages of dhw_page, which rows it
 * spans, and, when asked, a per-pixel map of the group whose ink is nearest.  No handle: errors are read through
 * dhw_last_error(NULL).  The call allocates nothing, synchronises nothing, never reads lens, slots or groups on the host and
 * can be captured into a graph; at most three launches, one fewer when labels_out is NULL and one fewer when scale > 0.  All
 * argument checks run before the first HIP call (DHW_ERR_ARG names the argument): N, L, P, H, W, lines_per_page,
 * margin_left, margin_top, pitch, line_width, scale and strokes by dhw_page's rules; 1 <= G <= 256; non-NULL groups /
 * boxes_out / spans_out / scale_out / workspace; labels_out (which may be NULL) and workspace 16-byte aligned, every other
 * pointer 4-byte aligned; workspace_bytes >= dhw_truth_workspace_bytes(N, L, G) (0 for an N, L or G outside the ranges).
 *
 * Line n, with lens[n] (L when lens is NULL) strokes and slot[n] = slots[n] (n when slots is NULL):
 *    1. Rules 1.-5. of dhw_render and 6.-9. of dhw_page, unchanged: pos = the prefix sums (in the line rasteriser's summation
 *       order: the positions have the raster's bits), lift, last, segment i is drawn iff 1 <= i < last and !lift[i],
 *       (xmin, xmax, ymin, ymax)_n = the box of the endpoints of drawn segments, which lines take part, ex_n, ey_n and s_n,
 *       the shared s (scale when scale > 0), the page slot[n] / lines_per_page and top_n = margin_top + (slot[n] %
 *       lines_per_page) pitch.  A device-side lens entry outside [1, L] is clamped to [0, L].
 *    2. Segment i runs from pos[i-1] to pos[i] and belongs to group g = groups[n,i].  A segment with g outside [0, G) is
 *       unassigned: it is ink, but belongs to no group.  groups[n,i] of a row that is not drawn is never read.
 *    3. The box of group g in stroke units: (gxmin, gxmax, gymin, gymax) = min / max over the endpoints of the drawn segments
 *       of the group.  Placement, fp32, every difference, product and sum one operation in the order written, none fused
 *       (rule 4 of dhw_paths):  oy = top_n + (pitch - ey_n s) 0.5;  left = margin_left + (gxmin - xmin_n) s;  right =
 *       margin_left + (gxmax - xmin_n) s;  top = oy + (ymax_n - gymax) s;  bottom = oy + (ymax_n - gymin) s.
 *       boxes_out[n,g] = (left, top, right, bottom).
 *    4. spans_out[n,g] = (first drawn row of the group, its last drawn row + 1, its number of drawn segments).  The rows
 *       between the first and the last need not all be the group's: groups may interleave.
 *    5. A group without a drawn segment, and every group of a line that takes no part, has zeros in both outputs.
 *    6. scale_out[0] = s.
 *    7. labels_out, when not NULL.  Pixel centres, the placement of the segments and the squared distance d2 from a centre to
 *       a segment are those of rule 12 of dhw_page, in the same tile-relative fp32 arithmetic.  Drawn segment i of line n has
 *       id = 1 + n G + g, or id = 0 when unassigned.  Pixel (r, c) of page p takes the id of the lexicographic minimum of
 *       (d2, id) over ALL drawn segments of the lines of that page, if sqrt(d2) < line_width/2 + 0.5 (exactly where dhw_page's
 *       coverage is above 0); otherwise 0.  Ink outside the page is clipped.  The lexicographic minimum is exact, commutative
 *       and associative: the map is bit-deterministic and independent of the order in which segments, chunks and lines are
 *       visited.  A pixel whose nearest point of the ink is a joint shared by two groups is at the same distance from both in
 *       exact arithmetic: there the fp32 rounding of the two distances decides, and only where they round to the same float
 *       does the smaller id win.  Such pixels form a wedge behind every joint between two groups; they are not rare.
 *    8. No global atomics and no float atomics.  The per-group min / max are integer min / max in LDS on an order-preserving
 *       integer image of the float, which is exact and commutative: the same call gives the same bits; line n inside any
 *       batch has the boxes and spans of line n alone (N = 1, the same slot, scale = the batch's s); boxes and spans do not
 *       depend on the order of the lines (the ids in the label map, 1 + n G + g, do by their definition). */
size_t dhw_truth_workspace_bytes(int N, int L, int G);
int dhw_truth(const float* strokes,      /* device f32 [N,L,3]                                             */
              const int32_t* lens,       /* DEVICE int32 [N] or NULL, any 1 <= n <= L                      */
              const int32_t* slots,      /* DEVICE int32 [N] or NULL (slot[n] = n)                         */
              const int32_t* groups,     /* DEVICE int32 [N,L]: the group of stroke row i of line n        */
              int N, int L, int G, int P, int H, int W, int lines_per_page,
              float margin_left, float margin_top, float pitch,      /* page pixels                        */
              float line_width, float scale,                         /* scale 0: automatic                 */
              float* boxes_out,          /* device f32 [N,G,4] = (left, top, right, bottom), page pixels   */
              int32_t* spans_out,        /* device i32 [N,G,3] = (first row, last row + 1, drawn segments) */
              int32_t* labels_out,       /* device i32 [P,1,H,W] or NULL                                   */
              float* scale_out,          /* device f32 [1]                                                 */
              void* workspace, size_t workspace_bytes, void* hip_stream);

/* Stroke encoder: raw pen trajectories (tablet points grouped into pen-down strokes, the IAM-OnDB lineStrokes data) -> the
 * model's (dx, dy, pen) rows, normalised and thinned as the reference's parse_strokes_xml + combine_strokes + pad_stroke_seq
 * prepare the training corpus.  No handle: errors are read through dhw_last_error(NULL).  The call allocates nothing,
 * synchronises nothing, makes no host read of counts and can be captured into a graph.  All argument checks run before the
 * first HIP call (DHW_ERR_ARG names the argument): 1 <= B <= 65535, 2 <= N <= 4096, 8 <= L <= 4096, 0 <= rounds <= 8,
 * max_abs > 0 and finite, non-NULL points / strokes_out / lens_out / status_out, points / strokes_out / workspace 16-byte
 * aligned, workspace_bytes >= dhw_encode_workspace_bytes(B, N).  A line of 4096 points stays in LDS, so the workspace size
 * is 0 at every shape today (and for a B or N outside the ranges) and workspace may then be NULL; the argument is there so
 * that a later layout can spill without a change of the ABI.
 *
 * Line b, with n = counts[b] (N when counts is NULL) points (x, y, end)[i], i < n; y grows DOWNWARD (tablet / IAM), end != 0
 * marks the last point of a pen-down stroke.  Points at or past n are never read.  All arithmetic is fp64 on values
 * converted from the f32 input, without fused multiply-add:
 *    1. Row i, 0 <= i < M with M = n - 1: d[i] = (x[i+1] - x[i], -(y[i+1] - y[i])), e[i] = (end[i+1] != 0).
 *    2. The pen column is e rolled by one: pen[0] = e[M-1], pen[i] = e[i-1] (the reference's convention: a 1 means the move
 *       TO this row is a jump).  The caller makes sure the last point of a line is marked as an end.
 *    3. Normalise: divide every dx and dy by s, the population standard deviation (ddof 0) of the 2M values dx and dy taken as
 *       ONE set, in two passes (the mean, then the mean squared deviation), each summed in a fixed tree; no float atomics.
 *    4. `rounds` times, with M the current row count: k = M / 5 (integer division; equal to the reference's int(M * 0.2) for
 *       every M <= 4096).  The pairs are (2j, 2j+1) for j < M / 2; an odd last row has no partner.
 *       v_j = |d[2j]| + |d[2j+1]| - |d[2j] + d[2j+1]| (Euclidean norms, sqrt(x x + y y)).  The k pairs that are smallest under
 *       the order (v_j, j) merge: on equal v the lower j goes first (the reference's argsort leaves ties at the cut
 *       unspecified).  A merged pair: d[2j] += d[2j+1], pen[2j] = (pen[2j] + pen[2j+1] > 0), row 2j+1 is deleted.  Unmerged
 *       rows keep their pen value.  After the deletions, rule 3 again on the new set.
 *    5. lens_out[b] = the final M (a function of n and rounds alone).
 *    6. status_out[b] is a bit set: 1: n < 2 or n > N.  2: a non-finite input among the n points, or a std that is 0 or
 *       non-finite at any normalisation (the values mean nothing from there on: the remaining rounds only shrink M, and
 *       bit 8 is not looked at).  4: final M > L.  8: max(|dx|, |dy|) over the final rows > max_abs (the reference's
 *       pad_stroke_seq uses 15).
 *    7. Status 0: rows i < M of strokes_out[b] are the f32 roundings of (dx, dy, pen); rows M <= i < L are (0, 0, 1), the
 *       reference's padding.
 *    8. Status non-zero: all L rows are (0, 0, 1) (the reference drops such a line); with bit 1 set lens_out[b] = 0 and no
 *       other bit is set.
 *    9. Row b of a batch equals the same line encoded alone, bit for bit, for any B, N and L that admit it. */
size_t dhw_encode_workspace_bytes(int B, int N);
int dhw_encode(const float* points,      /* device f32 [B,N,3] = (x, y, end)                     */
               const int32_t* counts,    /* DEVICE int32 [B] or NULL (every line has N points)   */
               int B, int N, int L, int rounds, float max_abs,
               float* strokes_out,       /* device f32 [B,L,3]                                   */
               int32_t* lens_out,        /* device [B]                                           */
               int32_t* status_out,      /* device [B]                                           */
               void* workspace, size_t workspace_bytes, void* hip_stream);

/* Writer-image preparation: B grey images of different sizes -> one f32 [B,1,H,W] batch that dhw_style_forward accepts, as
 * the reference's read_img (remove_whitespace, cv2.resize INTER_CUBIC to H rows) and its dataset's pad_img prepare a style
 * image.  No handle: errors are read through dhw_last_error(NULL).  The call allocates nothing, synchronises nothing, makes no
 * host read of sizes or of the crop boxes and can be captured into a graph.  All argument checks run before the first HIP call
 * (DHW_ERR_ARG names the argument): 1 <= B <= 65535, 1 <= Hin <= 4096, 16 <= Win <= 16384 and Win % 16 == 0, 8 <= H <= 512,
 * 8 <= W <= 4096 and W % 4 == 0, B H W < 2^31, 1 <= thresh <= 255, non-NULL images / img_out / status_out / workspace, images /
 * img_out / workspace 16-byte aligned (sizes / widths_out / boxes_out / status_out 4-byte), workspace_bytes >=
 * dhw_prep_workspace_bytes(B) (16 B bytes: the crop boxes; 0 for a B out of range).
 *
 * Image b, with (h, w) = sizes[b] (Hin, Win when sizes is NULL), lies in the top-left h x w corner of slot b of `images`:
 *    1. Pixels read.  Only pixels (r, c) with r < h and c < w are ever read.
 *    2. Crop box: the reference's remove_whitespace(img, thresh), remove_middle=False.  A pixel is dark iff its u8 value is
 *       < thresh.  r0, r1 = the first and last row holding a dark pixel, c0, c1 likewise for columns.  The crop is rows [r0, r1)
 *       and columns [c0, c1), upper bounds EXCLUSIVE as the reference slices: the last inked row and column are dropped.
 *       ch = r1 - r0, cw = c1 - c0.
 *    3. Output width: ow = (H cw) / ch, integer division (the reference's height * w // h).
 *    4. status_out[b] is a bit set: 1: h outside [1, Hin] or w outside [1, Win] (no other bit is then set and nothing of the
 *       image is read).  2: no dark pixel, or ch == 0, or cw == 0.  4: ow > W.  8: ow == 0.
 *    5. Resize: OpenCV's INTER_CUBIC conventions in fixed point.  For an axis with n_in source and n_out destination samples,
 *       destination index d has num = (2d + 1) n_in - n_out, den = 2 n_out, x0 = floor(num / den), t = (double)(num - x0 den) /
 *       (double)den (one fp64 division).  The Keys weights with a = -0.75 are evaluated in fp64 WITHOUT fused multiply-add:
 *       w0 = ((a (t+1) - 5a)(t+1) + 8a)(t+1) - 4a, w1 = (((a+2) t - (a+3)) t) t + 1, w2 = w1 at 1 - t, each product taken left
 *       to right.  c_k = rint(2048 w_k) for k = 0, 1, 2 (ties to even), c_3 = 2048 - c_0 - c_1 - c_2: a constant image stays
 *       constant.  The taps are the source indices clip(x0 - 1 + k, 0, n_in - 1) RELATIVE TO THE CROP: the border replicates
 *       the crop's own edge, pixels of the image outside the crop are not visible.  Horizontally n_in = cw, n_out = ow;
 *       vertically n_in = ch, n_out = H.
 *       value(e, d) = clamp((sum_j sum_k cy[e][j] cx[d][k] src[tap_y(e,j)][tap_x(d,k)] + 2^21) >> 22, 0, 255), exact integer
 *       arithmetic with an arithmetic shift, so the result does not depend on the order of evaluation (the separable form,
 *       horizontal pass first, gives the same integers).  sum |c| <= 2816 on each axis, so |sum| + 2^21 <= 255 * 2816^2 + 2^21
 *       < 2^31.
 *    6. Status 0: img_out[b,0,e,d] = (float)value(e, d) for d < ow and 255.0f for ow <= d < W (the reference's pad_img);
 *       widths_out[b] = ow, boxes_out[b] = (r0, r1, c0, c1).
 *    7. Status non-zero: all H W values are 255 and widths_out[b] = 0; boxes_out[b] holds the box when bit 1 is clear and there
 *       is ink, otherwise four zeros.
 *    8. Row b of a batch equals the same image prepared alone, bit for bit, for any B, Hin, Win and W that admit it.
 * PARITY WITH cv2 ITSELF IS UNPINNED: cv2 is not importable where this was written and its SIMD vertical pass is not
 * integer-exact; the scheme above is the deterministic statement this project pins (within one grey level of the float
 * resize of read_img: the coefficients are off by at most 3 / 4096). */
size_t dhw_prep_workspace_bytes(int B);
int dhw_prep(const uint8_t* images,   /* device u8 [B,Hin,Win], image b in the top-left h_b x w_b corner */
             const int32_t* sizes,    /* DEVICE int32 [B,2] = (h_b, w_b), or NULL: every image is Hin x Win */
             int B, int Hin, int Win, int H, int W, int thresh,
             float* img_out,          /* device f32 [B,1,H,W], grey levels 0..255 */
             int32_t* widths_out,     /* device [B] or NULL */
             int32_t* boxes_out,      /* device [B,4] = (r0, r1, c0, c1) or NULL */
             int32_t* status_out,     /* device [B] */
             void* workspace, size_t workspace_bytes, void* hip_stream);

/* Feature moments: the running sum and Gram matrix of pooled feature vectors in double precision, the statistics behind a
 * Frechet distance between two sets of style features.  No handle: errors are read through
 * dhw_last_error(NULL).  The call allocates nothing, synchronises nothing and can be captured into a graph.  All argument checks
 * run before the first HIP call (DHW_ERR_ARG names the argument): 1 <= N <= 16384, 1 <= S <= 64, D a multiple of 16 in
 * [16, 2048], N S D < 2^31, non-NULL and 16-byte aligned feat / sum / gram, ws_bytes >= dhw_moments_workspace_bytes(N, S, D)
 * (8 N D bytes: the pooled matrix; 0 for dimensions the entry refuses), ws non-NULL and 16-byte aligned.
 *    1. p[n][d] = (sum_s (double)feat[n][s][d]) / (double)S, s ascending from feat[n][0][d]: the mean over the S positions.
 *       S = 1 takes vectors that are pooled already.  Rows of feat at or past N are never read.
 *    2. sum[d] += sum_n p[n][d] and gram[i][j] += sum_n p[n][i] p[n][j], in double throughout; the Gram update runs on
 *       v_mfma_f64_16x16x4_f64 with n ascending, from the tile's current value.  The caller zeroes sum and gram once and keeps
 *       the sample count on the host.
 *    3. No atomics: every element has one owning workgroup, so the same call on the same state gives the same bits.  Only the
 *       upper triangle is computed; the owner writes the mirrored element too, so gram is bitwise symmetric on return (given a
 *       symmetric gram on entry).
 *    4. Non-finite inputs propagate as IEEE arithmetic has it. */
size_t dhw_moments_workspace_bytes(int N, int S, int D);
int dhw_moments_update(const float* feat,   /* device f32 [N,S,D]                     */
                       int N, int S, int D,
                       double* sum,         /* device f64 [D], in/out                 */
                       double* gram,        /* device f64 [D,D], in/out, both triangles */
                       void* ws, size_t ws_bytes, void* hip_stream);

/* Pairwise statistics of two sets of pooled feature vectors in double precision: what precision / recall (Kynkaanniemi et al.
 * 2019), density / coverage (Naeem et al. 2020), the kernel distance (unbiased MMD^2, cubic polynomial kernel) and a
 * nearest-neighbour search are made of.  No handle: errors are read through dhw_last_error(NULL).  The calls
 * allocate nothing, synchronise nothing and can be captured into a graph.  All argument checks run before the first HIP call
 * (DHW_ERR_ARG names the argument): 1 <= M, N <= 16384, D a multiple of 16 in [16, 2048], 1 <= k <= 8 and k < N, pointers
 * non-NULL (except where marked) and 16-byte aligned, ws_bytes >= dhw_pairs_workspace_bytes(M, N, D) (dhw_pairs_knn: of
 * (N, N, D); 0 for dimensions the entries refuse).
 *    1. dhw_pairs_pool: out[n][d] = (sum_s (double)feat[n][s][d]) / (double)S, s ascending: rule 1 of dhw_moments_update, the
 *       same kernel.  1 <= S <= 64, N S D < 2^31, rows of feat at or past N are never read.
 *    2. d2(i, j) = fmax(0, sq_i + sq_j - 2 dot_ij): sq the row's own squared norm in double, dot the inner product on
 *       v_mfma_f64_16x16x4_f64 with d ascending.  The M x N matrix is never written: it is reduced where it is computed.
 *    3. dhw_pairs_knn: radius2[i] = the k-th smallest of { d2(x_i, x_j) : j != i }.  j is excluded by index: a duplicate of
 *       row i counts, and gives radius 0.
 *    4. dhw_pairs_cover: count[m] = #{ j : d2(q_m, ref_j) <= radius2[j] }, nearest2[m] = min_j d2(q_m, ref_j), nearest_idx[m] =
 *       the smallest j attaining it.  radius2 and count are both given or both NULL; nearest_idx may be NULL.
 *    5. dhw_pairs_polysum: out[0] = sum_{i,j} (x_i . y_j + D)^3, without the pairs i == j when skip_diag != 0 (which needs
 *       M == N).  Dividing by D^3 and normalising is the caller's.
 *    6. No atomics: every output element has one writer and every sum a fixed order, so the same call on the same inputs gives
 *       the same bits.  The column range is split over workgroups and the partial results are merged in a fixed order; env
 *       DHW_PAIRS_SPLIT=<n> (read at each call; 0 or unset: automatic) forces the number of splits.  Rows at or past M / N are
 *       never read.  Inputs are assumed finite. */
int dhw_pairs_pool(const float* feat,   /* device f32 [N,S,D] */
                   int N, int S, int D,
                   double* out,         /* device f64 [N,D]   */
                   void* hip_stream);
size_t dhw_pairs_workspace_bytes(int M, int N, int D);
int dhw_pairs_knn(const double* x,      /* device f64 [N,D] */
                  int N, int D, int k,
                  double* radius2,      /* device f64 [N]   */
                  void* ws, size_t ws_bytes, void* hip_stream);
int dhw_pairs_cover(const double* q,          /* device f64 [M,D]        */
                    int M,
                    const double* ref,        /* device f64 [N,D]        */
                    int N, int D,
                    const double* radius2,    /* device f64 [N] or NULL  */
                    int32_t* count,           /* device i32 [M] or NULL  */
                    double* nearest2,         /* device f64 [M]          */
                    int32_t* nearest_idx,     /* device i32 [M] or NULL  */
                    void* ws, size_t ws_bytes, void* hip_stream);
int dhw_pairs_polysum(const double* x,   /* device f64 [M,D] */
                      int M,
                      const double* y,   /* device f64 [N,D] */
                      int N, int D, int skip_diag,
                      double* out,       /* device f64 [1]   */
                      void* ws, size_t ws_bytes, void* hip_stream);

/* Dynamic time warping (DTW) between every line of a set a and every line of a set b, in stroke space: a distance that sees
 * pen order, speed and lifts and needs no trained network.  No handle: errors are read through
 * dhw_last_error(NULL).  The call allocates nothing, synchronises nothing and can be captured into a graph.  All argument
 * checks run before the first HIP call (DHW_ERR_ARG names the argument): 1 <= M, N <= 16384 and M N <= 2^26; 1 <= La, Lb <=
 * 1024; 1 <= F <= 4; skip_diag only with M == N; at least one of dist_out / steps_out / nearest_out; nearest_idx only together
 * with nearest_out; a, b and ws non-NULL; every non-NULL pointer 16-byte aligned; ws_bytes >= dhw_dtw_workspace_bytes(M, N,
 * La, Lb, F) = M N sizeof(float) rounded up to a multiple of 16 (the matrix the nearest pass reads when dist_out is NULL), and 0
 * for dimensions the entry refuses.
 *
 * Pair (p, q), with n = lens_a[p] (La when lens_a is NULL) and m = lens_b[q] (Lb when lens_b is NULL):
 *    1. Rows of a[p] at or past n and rows of b[q] at or past m are never read, whatever they hold.
 *    2. c(i,j) = sum_{f<F} (a[p][i][f] - b[q][j][f])^2: the difference, the product and the sum over f ascending are fp32
 *       operations of their own; there is no fused multiply-add.
 *    3. D(0,0) = c(0,0) and K(0,0) = 1.
 *    4. Otherwise D(i,j) = c(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)) in fp32, over the predecessors that exist.
 *    5. The predecessor is the first of (i-1,j-1), (i-1,j), (i,j-1), in that order, that attains the minimum;
 *       K(i,j) = K(predecessor) + 1: the number of cells on the warping path.
 *    6. dist = D(n-1,m-1) and steps = K(n-1,m-1).  With normalize != 0, dist is divided by (float)steps in one correctly
 *       rounded fp32 division.
 *    7. A length outside [1, La] (or [1, Lb]) gives dist = +inf and steps = 0 for every pair of that line.
 *    8. nearest_out[p] = the smallest dist over q (q != p with skip_diag != 0), nearest_idx[p] = the smallest q attaining it;
 *       +inf and -1 when no pair of p is finite.
 *    9. No atomics and one writer per output element: the same call gives the same bits, and pair (p, q) gives the same bits
 *       alone (M = N = 1) as inside any batch.
 *   10. Non-finite features are the caller's business: no access leaves the buffers, nothing else is promised for them. */
size_t dhw_dtw_workspace_bytes(int M, int N, int La, int Lb, int F);
int dhw_dtw(const float* a, const int32_t* lens_a, int M, int La,     /* device f32 [M,La,F]; DEVICE int32 [M] or NULL */
            const float* b, const int32_t* lens_b, int N, int Lb,     /* device f32 [N,Lb,F]; DEVICE int32 [N] or NULL */
            int F, int normalize, int skip_diag,
            float* dist_out,        /* device f32 [M,N] or NULL */
            int32_t* steps_out,     /* device int32 [M,N] or NULL */
            float* nearest_out,     /* device f32 [M] or NULL */
            int32_t* nearest_idx,   /* device int32 [M] or NULL; only together with nearest_out */
            void* ws, size_t ws_bytes, void* hip_stream);

/* Reuse of the text side across calls.  The text side of the sampler (TextStyleEncoder and every layer's text K / V, for all T
 * steps) depends on text, style, T and the weights only.  A dhw_sample / dhw_sample_ragged / dhw_sample_cond call whose text and
 * style hold the same BITS as the previous such call's on this handle, at the same B, Lt, T and t_start, with unchanged weights
 * and switches, finds that result still in the handle and does not evaluate it again; its samples are bit-identical to a call
 * that does.  Contents are compared on the device at every call, so tensors edited in place are seen.  The first call, and a call
 * with other prompts or styles, costs what it always did.  bf16 handles, T <= 64; env DHW_PLANE_REUSE=0 at dhw_create turns the
 * reuse off.  This entry synchronises the device and reports: last = 1 when the most recent such call reused the text side, calls
 * = how many were enqueued, reused = how many of them reused it.  Any pointer may be NULL. */
int dhw_debug_plane_reuse(dhw_handle*, int* last, long* calls, long* reused);

/* Host-only: beta_i = 0.02 + exp(linspace(ln 1e-5, ln 0.4, T)), abar = cumprod(1-beta), fp32. */
int dhw_schedule(int T, float* beta_out, float* alpha_bar_out);

/* Algorithmic work of one denoiser call per sample at (L, Lt): FLOPs and the
 * block-boundary activation bytes; used by bench.py. */
int dhw_work(dhw_handle*, int L, int Lt, double* flops_out, double* bytes_out);

const char* dhw_last_error(dhw_handle*);   /* valid until the next call on the handle; NULL handle -> global */
const char* dhw_version(void);
void dhw_destroy(dhw_handle*);

#ifdef __cplusplus
}
#endif
#endif /* DHW_H */
