/* dhw_debug.h — test / measurement hooks of libdhw_hip.so (not part of the
 * drop-in boundary; used by tests/ and bench.py only). */
#ifndef DHW_DEBUG_H
#define DHW_DEBUG_H

#include "dhw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Copy the named intermediate activation of the LAST dhw_forward call to the
 * host as fp32, C-last [B, rows, cols].  Names follow the reference's module
 * names ("enc1", "enc3", "att_layers.0", "text_style_model", "skip_conv3",
 * "sigma_ffn", "input_dense", "att_dense", ...; "enc1.pool", "enc3.pool",
 * "enc5.pool" are the AvgPool1d side outputs).  Only buffers the last call
 * wrote have a name: after dhw_sample, whose dec1 keeps its activation in LDS
 * for the fused heads, "dec1" is refused.  Synchronises the device.
 * Returns the number of floats written, or a negative dhw_status. */
int64_t dhw_debug_read(dhw_handle*, const char* name, float* host_dst, int64_t max_floats,
                       int64_t shape_out[3]);

/* After dhw_forward the text keys and values of every EncoderLayer are activations too: "<layer>.k1" [B, Lt, d] and
 * "<layer>.v1", reported AS STORED - rows [B, Lt, d] where the fused bf16 EncoderLayer kernels read them, else the
 * transposed V^T [B, d, lpadT] (lpadT = the handle's max_Lt rounded up to 32; columns >= Lt are not part of the call). */

/* The all-steps text plane of dhw_sample (one slot per (step, prompt) pair), as the LAST dhw_sample* call left it in
 * workspace `workspace_slot` (0 unless dhw_set_streams split the batch), copied to the host as fp32 [pairs, rows, cols].
 * Names: "text_style_model" [pairs, Lt, 2 c2], "<layer>.k1" [pairs, Lt, d], "<layer>.v1" (as above: [pairs, Lt, d] or
 * [pairs, d, lpadT]).  Slot k * Bs + b of a chunk of up to 64 steps holds step (first + chunk start + k) of prompt b; a later
 * chunk overwrites the slots from 0 on, and every slot the call's chunking wrote is returned: pairs = min(64, steps run) * Bs.
 * DHW_ERR_STATE where the handle keeps no plane (DHW_PLANE=0), no sample call has run, or the last call replayed a graph
 * captured before the plane was re-allocated.  Synchronises the device; reads only (the plane-reuse tag is left alone).
 * Returns the number of floats written, or a negative dhw_status. */
int64_t dhw_debug_read_plane(dhw_handle*, int workspace_slot, const char* name, float* host_dst, int64_t max_floats,
                             int64_t shape_out[3]);

/* Per-kernel timing: when enabled every launch is bracketed by HIP events on
 * the launch stream (graph replay is disabled while profiling). */
int dhw_profile_enable(dhw_handle*, int on);
int dhw_profile_reset(dhw_handle*);
/* Resolve pending events; returns the number of distinct kernel labels. */
int dhw_profile_count(dhw_handle*);
int dhw_profile_get(dhw_handle*, int i, const char** label, double* total_ms, int64_t* launches,
                    double* flops_per_launch_sum, double* bytes_per_launch_sum);

/* Number of prompt sub-batches dhw_sample runs concurrently (parallel graph branches on side streams);
 * clamped to the count allocated at create (env DHW_STREAMS, default 1).  Returns the value in effect. */
int dhw_set_streams(dhw_handle*, int n);

/* Use (1) or bypass (0) hipGraph replay of the sampling loop. Default 1. */
int dhw_set_graph(dhw_handle*, int on);
/* Number of dhw_sample shapes that run every denoiser call as ONE persistent launch (csrc/persist.h; OFF by default — it measured
   slower than the eleven launches, DESIGN 13.3 — env DHW_PERSIST=1 at dhw_create turns that form on).  0 = every call so far was
   launched kernel by kernel. */
int dhw_debug_persist_plans(dhw_handle*);
/* Diagnostics (DHW_PERSIST_TRACE=1 at dhw_create): 100 MHz time stamps of the last persistent step of the last dhw_sample call,
   [workgroup][16 phases][4] = {ticket drawn, inputs ready, body done, (phase 0: kernel entry; phase 1: exit | xcc << 56)}.
   Returns the number of workgroups, 0 without a trace buffer. */
int dhw_debug_persist_trace(dhw_handle*, unsigned long long* host_dst, int64_t max_words);

/* Teacher forcing of dhw_sample, for long-schedule parity tests (the random-init reverse process grows by 1/sqrt(1 - beta)
 * per step, so a free-running T = 1000 trajectory leaves every meaningful range; SURVEY 7 "hard parts"): with every > 0 the
 * next dhw_sample calls run eagerly and, in front of step k*every (k = 1, 2, ... while k*every < T), copy the state x
 * [B,L,2] reached so far to capture_dev[k-1] and continue from reset_dev[k-1] (device buffers of (T-1)/every x [B,L,2] floats,
 * owned by the caller, alive until the calls have completed).  every = 0 switches it off. */
int dhw_debug_set_teacher(dhw_handle*, const float* reset_dev, float* capture_dev, int every);

/* The device noise generator on its own: the N(0,1) draws of `B` samples x `L` positions x 2 for sampler iteration
 * `iter` (-1 = x_T, k >= 0 = the draw step k adds) under (seed, first_sample), copied to host_dst [B,L,2].
 * Exactly the values dhw_sample(noise = NULL) consumes.  Synchronises the device. */
int dhw_debug_randn(dhw_handle*, uint64_t seed, int64_t first_sample, int B, int L, int iter, float* host_dst);

/* The logical workgroup id the fused kernels derive from blockIdx (csrc/dhw_common.h xcd_swizzle): a bijection of
 * [0, nwg) that gives each of the 8 XCDs a contiguous id range.  Host-side copy for tests; needs no device. */
int dhw_debug_xcd_swizzle(int block_id, int nwg);

/* The self-attention stage of EncoderLayer `layer` (0 = enc3, 1 = enc5, 2 + i = att_layers.i) timed on its own, on the
 * activations the last dhw_forward left in the workspace: enc_bc_kernel launched `iters` times with the stage and `iters`
 * times with the stage skipped, mean launch time of each in microseconds (HIP events on `hip_stream`); flops_out = the
 * stage's QK^T + PV FLOPs, 4 B Lk^2 d.  bf16 handles with the fused kernels only; synchronises the stream. */
int dhw_debug_attention_time(dhw_handle*, int layer, int iters, double* us_with, double* us_without, double* flops_out,
                             void* hip_stream);

/* Raise a C++ exception inside the guarded body of an entry point: kind 1 = std::out_of_range (a std::map::at miss), 2 =
 * std::bad_alloc, 3 = a non-std exception.  Returns DHW_ERR_INTERNAL with the message in dhw_last_error(handle) — the test of
 * "nothing throws across the ABI" (include/dhw.h).  Needs no device; the handle may be NULL (message in the global slot). */
int dhw_debug_raise(dhw_handle*, int kind);

/* The host half of the text-plane reuse decision (csrc/sampler/plane_tag.h), without a handle or a device: 1 when a call
 * described by `call` may reuse the plane described by `resident`, else 0.  Both are {valid, B, nstreams, Lt, S, T, t_start, weights
 * generation, FiLM table identity, plane allocation generation}; gates: bit 0 = DHW_PLANE_REUSE on, bit 1 = the all-steps plane in
 * use, bit 2 = fused bf16 text-side kernels serve the call. */
int dhw_debug_plane_tag(const int64_t resident[10], const int64_t call[10], int gates);

/* The tile plan of the stroke kernels (csrc/plan/tile_plan.h): which compiled kernel variant a launch runs.  None of
 * these needs a device or a handle.  Variants are reported as their template arguments:
 *   ConvBlock     {f32, BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP, output rows per tile}      (convblock_kernel, csrc/convblock.hip)
 *   EncoderLayer  {f32, DM, BM}                                                               (enc_a_kernel / enc_bc_kernel, csrc/enclayer.hip)
 * prec: 0 = bf16, 1 = fp32.
 *
 * dhw_debug_conv_plan: the variant of one ConvBlock launch at (B, L, Cin, Cout); up_cin != 0 = a decoder block with the fused input
 * stage over a skip activation of that width; chain != 0 = the block continues into the next EncoderLayer's first half.  A pure
 * function of its arguments: the switches come in as knobs = {wgs, bm, occ, pp, asym, tight, rt} (the environment unset:
 * {256, 0, 0, 0, 1, 1, 0}; bm / occ: 0 = not forced), never from the environment.  out[0] = the variant's index in the compiled
 * list, or -1 = the launch is refused; out[1..11] = the variant. */
int dhw_debug_conv_plan(int prec, int B, int L, int Cin, int Cout, int up_cin, int chain, const int64_t knobs[7], int out[12]);
/* The same for both halves of an EncoderLayer of width d at (B, Lk) with EncLayerParams.bm_min; knobs = {forced row tile, wgs}
 * ({0, 256}).  out = {index in the compiled list or -1, f32, DM, BM}. */
int dhw_debug_enc_plan(int prec, int d, int B, int Lk, int bm_min, const int64_t knobs[2], int out[4]);
/* gemm_tile_for (csrc/gemm.hip) for a GEMM of B samples x L rows x N columns: out = {row tile, column tile}. */
int dhw_debug_gemm_plan(int prec, int B, int L, int N, int n_store, int ln, int out[2]);
/* The switch values the library reads from the environment right now: {DHW_CONV_WGS, _BM, _OCC, _PP, _ASYM, _TIGHT, _RT, _STAGGER,
 * DHW_ENC_BM as it holds for d = 192, 256, 384, DHW_ENC_WGS}.  ASYM / TIGHT / RT are frozen by the first read in the process, this
 * call included. */
int dhw_debug_tile_knobs(int64_t out[12]);
/* Row i of the compiled list of kind 0 (ConvBlock: out = the 11 values above) or 1 (EncoderLayer: out = {f32, DM, BM, whether
 * fits() holds, i.e. the kernels exist, chain modes of has_chain(): bit 0 = mode 1, bit 1 = mode 2}).  Returns the length of the
 * list (for any i; out may be NULL), or a negative dhw_status. */
int dhw_debug_tile_variants(int kind, int i, int out[11]);

#ifdef __cplusplus
}
#endif
#endif
