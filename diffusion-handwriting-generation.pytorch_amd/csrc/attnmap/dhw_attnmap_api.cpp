// dhw_attnmap_api.cpp — C-ABI of the attention maps (include/dhw.h: dhw_attention, dhw_attention_shape): one denoiser call
// (sampler/sample.cpp: forward_enqueue), the layer's Q projection over the input that call left in the workspace (the generic
// GEMM, "attnmap.q"), and the map kernel over that Q and the call's text keys — eagerly on the caller's stream.  Nothing here
// touches h->d_seed, the sampler's staging buffers or its graph cache.
#include "../sampler/denoiser.h"
#include "attnmap.h"

// heads of EncoderLayer li (0 = enc3, 1 = enc5, 2 + i = att_layers.i) and the shift from the full length to its rows
static int layer_heads(int li) { return li == 0 ? 3 : li == 1 ? 4 : 6; }
static int layer_shift(int li) { return li == 0 ? 1 : li == 1 ? 2 : 3; }

static int check_layer(dhw_handle* h, const char* fn, int layer) {
  if (layer < 0 || layer >= 2 + h->dims.num_layers)
    return fail(h, DHW_ERR_ARG, "%s: layer = %d must lie in [0, %d) (0 = enc3, 1 = enc5, 2 + i = att_layers.i)", fn, layer, 2 + h->dims.num_layers);
  return 0;
}

static int shape_impl(dhw_handle* h, int layer, int L, int* heads_out, int* Lq_out) {
  const char* fn = "dhw_attention_shape";
  // a NULL handle answers for any model: only the limits that belong to a handle (its layer count, its max_L) are skipped
  if (h) {
    if (int rc = check_layer(h, fn, layer)) return rc;
  } else if (layer < 0) {
    return fail(nullptr, DHW_ERR_ARG, "%s: layer = %d must not be negative (0 = enc3, 1 = enc5, 2 + i = att_layers.i)", fn, layer);
  }
  if (L < 8 || L % 8 || (h && L > h->dims.max_L)) return fail(h, DHW_ERR_ARG, "%s: L = %d must be a multiple of 8, at least 8%s", fn, L, h ? " and at most the handle's max_L" : "");
  if (heads_out) *heads_out = layer_heads(layer);
  if (Lq_out) *Lq_out = L >> layer_shift(layer);
  return 0;
}

static int attention_impl(dhw_handle* h, const float* strokes, const int64_t* text, const float* sigma, const float* style, int B, int L, int Lt,
                          const int32_t* lens, int layer, float* probs_out, float* mean_out, int32_t* token_out, float* eps_out, float* pen_out,
                          void* hip_stream) {
  const char* fn = "dhw_attention";
  // every check answers before dhw_finalize, the first thing that can touch HIP (include/dhw.h, rule 5)
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  if (!strokes || !text || !sigma || !style || !eps_out || !pen_out)
    return fail(h, DHW_ERR_ARG, "%s: null pointer (%s)", fn, !strokes ? "strokes" : !text ? "text" : !sigma ? "sigma" : !style ? "style" : !eps_out ? "eps_out" : "pen_out");
  int rc = eager_check(h, fn, B, L, Lt, lens, true);   // (the forward entry's shape message, under this entry's name)
  if (rc) return rc;
  if ((rc = check_layer(h, fn, layer))) return rc;
  if (!probs_out && !mean_out && !token_out) return fail(h, DHW_ERR_ARG, "%s: probs_out, mean_out and token_out are all NULL: nothing to write", fn);
  if (((uintptr_t)probs_out | (uintptr_t)mean_out) & 15)
    return fail(h, DHW_ERR_ARG, "%s: %s must be 16-byte aligned", fn, ((uintptr_t)probs_out & 15) ? "probs_out" : "mean_out");
  if (Lt > ATTNMAP_MAX_LT) return fail(h, DHW_ERR_ARG, "%s: Lt = %d is more than the map kernel holds (%d)", fn, Lt, ATTNMAP_MAX_LT);

  EagerCall ec;
  if ((rc = eager_begin(h, B, L, Lt, lens, hip_stream, &ec))) return rc;   // (leaves dhw_sample's text plane alone: forward_enqueue)
  auto& [st, dlens, c] = ec;
  if ((rc = forward_enqueue(h, strokes, text, sigma, style, B, L, Lt, eps_out, pen_out, st, dlens))) return rc;

  const EncLayerW& w = h->el[(size_t)layer];
  const int H = layer_heads(layer), sh = layer_shift(layer), Lq = L >> sh, d = w.d;
  if (w.heads != H || d != H * ATTNMAP_D) return fail(h, DHW_ERR_INTERNAL, "%s: layer %d has %d heads over %d channels, the map kernel expects %d x %d", fn, layer, w.heads, d, H, ATTNMAP_D);
  // the Q projection reads the call's FiLM rows and lengths, as the forward's launches did
  c.film_bs = 2L * h->film_tot;
  c.lens = dlens;
  // the layer's input, as the forward left it (each a debug tap of that call, in the fused and the one-launch-per-GEMM path)
  const void* x = layer == 0 ? CBB(c, CB_ENC2, out) : layer == 1 ? CBB(c, CB_ENC4, out) : layer == 2 ? WS(c, att_dense) : ELB(c, layer - 1, out);
  void* q = ELB(c, layer, q1);   // [max_B * max_Lq, d]: the fused path leaves it unused, the other one writes these very values
  const void* k = need(c, c.ws->el[(size_t)layer].t.k1, "k1");
  if (c.err) return c.err;
  {  // q1 = Wq(x + PE), the launch of denoiser.cpp's "enc.q_cross"
    GemmParams g{};
    g.nseg = 1;
    g.B = B; g.L = Lq; g.N = d; g.n_store = d;
    g.film_bs = c.film_bs; g.film_div = c.film_div;
    g.seg[0] = GemmSeg{x, w.w_q1, d, 1, 0};
    g.bias0 = w.b_q1;
    g.posb = w.pb_q1;
    g.posb_cols = d;
    g.out = q;
    g.lens = dlens; g.lsh = sh;
    run_gemm(c, "attnmap.q", g);
    if (c.err) return c.err;
  }
  AttnMapParams p{};
  p.Q = q; p.ldq = d;
  p.K = k; p.ldk = d;
  p.text = text;
  p.lens = dlens; p.lsh = sh;
  p.B = B; p.H = H; p.Lq = Lq; p.Lt = Lt;
  p.probs = probs_out; p.mean = mean_out; p.token = token_out;
  RUN_SMALL(c, "attnmap", launch_attnmap(h->prec, p, st));
  return c.err;
}

extern "C" {

int dhw_attention_shape(dhw_handle* h, int layer, int L, int* heads_out, int* Lq_out) {
  DHW_GUARD(h, "dhw_attention_shape", int, { return shape_impl(h, layer, L, heads_out, Lq_out); });
}

int dhw_attention(dhw_handle* h, const float* strokes, const int64_t* text, const float* sigma, const float* style, int B, int L, int Lt,
                  const int32_t* lens, int layer, float* probs_out, float* mean_out, int32_t* token_out, float* eps_out, float* pen_out, void* hip_stream) {
  DHW_GUARD(h, "dhw_attention", int, {
    return attention_impl(h, strokes, text, sigma, style, B, L, Lt, lens, layer, probs_out, mean_out, token_out, eps_out, pen_out, hip_stream);
  });
}

}  // extern "C"
