// sampler/denoiser.cpp — the denoiser launch sequence (== DiffusionModel.forward, reference model.py:121-182): fused block
// kernels, the one-launch-per-GEMM path, and record mode for the persistent step kernel (persist.h).
#include <cstdlib>

#include "denoiser.h"

// level of a stroke-side launch: L_full >> shift == L (full, /2, /4, /8)
static int level_shift(int L_full, int L) {
  int k = 0;
  while ((L << k) < L_full) ++k;
  return k;
}

// append one phase of the persistent per-step kernel (record mode)
static void rec_phase(Ctx& c, int kind, int L, const ConvBlockParams* cb, const EncLayerParams* el, const EncChain* nx) {
  int rows = 0, lv = 0;
  if (!step_kind_geometry(kind, L, &rows, &lv) || (int)c.rec->size() >= STEP_MAX_PHASES) { c.rec_fail = true; return; }
  StepPhase ph{};
  ph.kind = kind;
  ph.rows = rows;
  ph.tps = (lv + rows - 1) / rows;
  if (cb) ph.cb = *cb;
  if (el) ph.el = *el;
  if (nx) ph.nx = *nx;
  c.rec->push_back(ph);
}

void* need(Ctx& c, void* p, const char* what) {
  if (!p && !c.err) c.err = fail(c.h, DHW_ERR_INTERNAL, "internal: workspace buffer '%s' was never allocated", what);
  return p;
}

static GemmParams gp_base(const Ctx& c, int L, int N) {
  GemmParams p{};
  p.nseg = 1;
  p.B = c.B;
  p.L = L;
  p.N = N;
  p.n_store = N;
  p.film_bs = c.film_bs;
  p.film_div = c.film_div;
  return p;
}
// a GEMM of the stroke path at a level of L rows per sample: in a ragged batch it carries the per-sample lengths
static GemmParams gp_stroke(const Ctx& c, int L, int N) {
  GemmParams p = gp_base(c, L, N);
  p.lens = c.lens;
  p.lsh = level_shift(c.L, L);
  return p;
}
// All-steps text plane: a GEMM with no per-sample structure (no position bias, no transposed-V output) can see each
// sampler step as ONE long "sample" of film_div*L rows sharing one FiLM row, so 64-row tiles run across prompts.
// Measured slower than per-prompt 32-row tiles (29.60 vs 29.28 ms/step: the 64x384 LayerNorm tile runs at one wave per
// SIMD), so it is opt-in (DHW_FLAT_TEXT=1).
static GemmParams gp_text(const Ctx& c, int L, int N) {
  GemmParams p = gp_base(c, L, N);
  static const bool flat = getenv("DHW_FLAT_TEXT") && atoi(getenv("DHW_FLAT_TEXT")) != 0;
  if (c.film_div > 1 && flat) {
    p.B = c.B / c.film_div;
    p.L = L * c.film_div;
    p.film_div = 1;
  }
  return p;
}
static void set_film(const Ctx& c, GemmParams& p, int off, int mode) {
  p.gam = c.film + off;
  p.bet = c.film + c.h->film_tot + off;
  p.film_mode = mode;
}
static double gemm_flops(const GemmParams& p) {
  double k = 0;
  for (int s = 0; s < p.nseg; ++s) k += (double)p.seg[s].C * p.seg[s].taps;
  return 2.0 * p.B * p.L * p.N * k;
}
static double gemm_bytes(const dhw_handle* h, const GemmParams& p) {   // algorithmic: activations in + out once, weights once
  double b = 0;
  for (int s = 0; s < p.nseg; ++s) b += (double)p.B * p.L * p.seg[s].C * h->es + (double)p.N * p.seg[s].C * p.seg[s].taps * h->es;
  b += (double)p.B * p.L * p.N * (p.out_f32 ? 4 : h->es);
  if (p.res1) b += (double)p.B * p.L * p.N * h->es;
  if (p.res2) b += (double)p.B * p.L * p.N * h->es / (p.res2_half ? 2 : 1);
  if (p.pool) b += (double)p.B * p.L * p.N * h->es / 2;
  return b;
}
void run_gemm(Ctx& c, const char* label, const GemmParams& p) {
  if (c.rec) { c.rec_fail = true; return; }
  if (c.err) return;
  Launch l(c.h, c.st, label, gemm_flops(p), gemm_bytes(c.h, p));
  GemmParams q = p;
  if (q.ln) q.ln_n = true_width(c.h, q.N);
  hipError_t e = q.lens ? launch_gemm_ragged(c.h->prec, q, c.st) : launch_gemm(c.h->prec, q, c.st);
  if (e != hipSuccess) c.err = fail(c.h, DHW_ERR_HIP, "gemm %s: %s", label, hipGetErrorString(e));
}
static void run_attn(Ctx& c, const char* label, const AttnParams& p) {
  if (c.rec) { c.rec_fail = true; return; }
  if (c.err) return;
  Launch l(c.h, c.st, label, 4.0 * p.B * p.H * (double)p.Lq * p.Lk * p.D,
           (double)p.B * p.H * p.D * (2.0 * p.Lq + 2.0 * p.Lk) * c.h->es);
  hipError_t e = p.lens ? launch_attn_ragged(c.h->prec, p, c.st) : launch_attn(c.h->prec, p, c.st);
  if (e != hipSuccess) c.err = fail(c.h, DHW_ERR_HIP, "attn %s: %s", label, hipGetErrorString(e));
}

void tap(Ctx& c, int id, void* p, int rows, int cols, bool f32) {
  TapSlot& s = c.h->taps[id];
  s.t = Tap{p, rows, cols, f32};
  s.set = true;
}
void taps_clear(dhw_handle* h) {
  for (TapSlot& s : h->taps) s.set = false;
}

// decoder input produced inside the block: Upsample(low) + skip_conv(hskip)  (model.py:169-175)
struct UpIn { const void* hskip; const void* w; const float* b; int cin; const void* low; };

// cnn.py:64-87 as one fused launch (or three fused GEMM launches)
// chain: the EncoderLayer half the block's workgroups continue with (EncChain mode 1), or null; *chained reports
// whether the launch took it
// chain_auto: take the chain only where convblock_chain_auto says it pays for this launch geometry
static void conv_block(Ctx& c, int id, const ConvBlockW& w, const void* x, int L, void* out, bool out_f32,
                void* pool, const float* strokes = nullptr, const UpIn* up = nullptr, const EncChain* chain = nullptr,
                bool* chained = nullptr, bool chain_auto = false) {
  dhw_handle* h = c.h;
  const char* n = kConvName[id];
  if (h->fuse) {
    ConvBlockParams q{};
    q.strokes = strokes; q.in_w = h->in_w; q.in_b = h->in_b;
    if (up) { q.up_h = up->hskip; q.up_cin = up->cin; q.up_w = up->w; q.up_b = up->b; q.up_low = up->low; }
    q.x = x; q.B = c.B; q.L = L; q.Cin = w.cin; q.Cout = w.cout;
    q.w_c1 = w.w_c1; q.w_c2 = w.w_c2; q.w_fc = w.w_fc; q.w_skip = w.w_skip;
    q.b_c1 = w.b_c1; q.b_c2 = w.b_c2; q.b_fc = w.b_fc; q.b_skip = w.b_skip;
    q.film = c.film; q.film_bs = c.film_bs; q.film_tot = h->film_tot;
    q.f1 = w.f1; q.f2 = w.f2; q.f3 = w.f3;
    q.out = out; q.out_f32 = out_f32; q.pool = pool;
    q.lens = c.lens; q.lsh = level_shift(c.L, L);
    q.store = store_policy_of(h->store_policy, 0);
    if (c.fhp && id == CB_DEC1) {
      q.fuse_heads = 1;
      q.hp = *c.fhp;
      q.hp.w_out = h->out_w; q.hp.b_out = h->out_b; q.hp.w_pen = h->pen_w; q.hp.b_pen = h->pen_b;
      q.hp.L = L;
      q.out = nullptr;   // the fp32 activation never leaves LDS
    }
    if (c.rec) {
      // the phase kinds the persistent kernel is built with (persist.h): the reference's widths, the canonical row tiles
      const bool ch = chain && chain->mode == 1 && convblock_chain_supported(h->prec, q, *chain) && (!chain_auto || convblock_chain_auto(q));
      if (chained) *chained = ch;
      int kind = -1;
      if (id == CB_ENC1 && strokes && !up) kind = PK_CONV_ENC1;
      else if (id == CB_ENC2 && ch && !up && !strokes) kind = PK_CONV_ENC2A;
      else if (id == CB_ENC4 && !(chain && chain->mode) && !up && !strokes) kind = PK_CONV_ENC4;
      else if (id == CB_DEC3 && up) kind = PK_CONV_DEC3;
      else if (id == CB_DEC2 && up) kind = PK_CONV_DEC2;
      else if (id == CB_DEC1 && up && q.fuse_heads) kind = PK_CONV_DEC1;
      if (kind < 0 || h->prec != PREC_BF16 || (L & 1)) { c.rec_fail = true; return; }
      rec_phase(c, kind, c.L, &q, nullptr, ch ? chain : nullptr);
      return;
    }
    if (!c.err) {
      const double rows = (double)c.B * L;
      const double upf = up ? 3.0 * up->cin * w.cin : 0.0;   // skip_conv MACs per row
      const bool ch = chain && chain->mode && convblock_chain_supported(h->prec, q, *chain) && (!chain_auto || convblock_chain_auto(q));
      if (chained) *chained = ch;
      const double dd = w.cout;
      const double chf = ch ? 2.0 * rows * dd * dd * 5 + 4.0 * rows * c.Lt * dd : 0.0, chb = ch ? rows * dd * 4 * h->es + 5.0 * dd * dd * h->es : 0.0;
      Launch l(h, c.st, ch ? "convblock.fused+a" : "convblock.fused", 2.0 * rows * (4.5 * w.cin * w.cout + 2.5 * w.cout * w.cout + upf) + chf,
               rows * ((up ? up->cin + 0.5 * w.cin : w.cin) * h->es + w.cout * (out_f32 ? 4.0 : (double)h->es) * (pool ? 1.5 : 1.0)) +
                   (4.5 * w.cin * w.cout + 2.5 * w.cout * w.cout + upf) * h->es + chb);
      // (a handle with another store policy than the compiled-in default: the launchers that read it from the parameter blocks)
      const bool pol = h->store_policy != DHW_STORE_DEFAULT;
      hipError_t e = q.lens ? (ch ? launch_convblock_chain_ragged(h->prec, q, *chain, c.st) : launch_convblock_ragged(h->prec, q, c.st))
                     : pol  ? (ch ? launch_convblock_chain_policy(h->prec, q, *chain, c.st) : launch_convblock_policy(h->prec, q, c.st))
                            : (ch ? launch_convblock_chain(h->prec, q, *chain, c.st) : launch_convblock(h->prec, q, c.st));
      if (e != hipSuccess) c.err = fail(h, DHW_ERR_HIP, "convblock %s: %s", n, hipGetErrorString(e));
    }
    // (dec1 with the heads fused in keeps its activation in LDS: there is no buffer to read, the tap stays unset)
    if (q.out) tap(c, tap_conv(id), out, L, w.cout, out_f32);
    if (pool) tap(c, TAP_POOL1, pool, L / 2, w.cout);   // (enc1 is the only ConvBlock with a pooled side output)
    return;
  }
  if (c.rec) { c.rec_fail = true; return; }
  {  // h1 = SiLU(FiLM1(conv1(SiLU(x))))
    GemmParams p = gp_stroke(c, L, w.cout / 2);
    p.seg[0] = GemmSeg{x, w.w_c1, w.cin, 3, 1};
    p.bias0 = w.b_c1;
    set_film(c, p, w.f1, 1);
    p.silu_out = 1;
    p.out = CBB(c, id, h1);
    run_gemm(c, "convblock.conv1", p);
  }
  {  // h2 = SiLU(FiLM2(conv2(h1)))
    GemmParams p = gp_stroke(c, L, w.cout);
    p.seg[0] = GemmSeg{CBB(c, id, h1), w.w_c2, w.cout / 2, 3, 0};
    p.bias0 = w.b_c2;
    set_film(c, p, w.f2, 1);
    p.silu_out = 1;
    p.out = CBB(c, id, h2);
    run_gemm(c, "convblock.conv2", p);
  }
  {  // out = FiLM3(fc(h2)) + conv_skip(x)
    GemmParams p = gp_stroke(c, L, w.cout);
    p.nseg = 2;
    p.seg[0] = GemmSeg{CBB(c, id, h2), w.w_fc, w.cout, 1, 0};
    p.seg[1] = GemmSeg{x, w.w_skip, w.cin, 3, 0};
    p.bias0 = w.b_fc;
    p.bias1 = w.b_skip;
    set_film(c, p, w.f3, 2);
    p.out = out;
    p.out_f32 = out_f32;
    p.pool = pool;
    run_gemm(c, "convblock.fc_skip", p);
  }
  tap(c, tap_conv(id), out, L, w.cout, out_f32);
  if (pool) tap(c, TAP_POOL1, pool, L / 2, w.cout);
}

// the per-call text keys / values of layer li as dhw_debug_read reports them: v1 as it is stored (handle.h v_rows)
static void tap_text_kv(Ctx& c, int li, const EncLayerW& w, bool rows) {
  if (c.planeT) return;   // (the all-steps plane: dhw_debug_read_plane)
  tap(c, tap_el(li, 3), ELT(c, li, k1), c.Lt, w.d);
  if (rows) tap(c, tap_el(li, 4), ELT(c, li, vt1), c.Lt, w.d);
  else tap(c, tap_el(li, 4), ELT(c, li, vt1), w.d, c.h->lpadT);
}

// model.py:37-58.  The text-side projections (tl, k1, vt1) are produced by enc_layer_text.
static void enc_layer_text(Ctx& c, int li, const EncLayerW& w) {
  dhw_handle* h = c.h;
  const int dt = 2 * h->dims.c2;
  {  // tl = FiLM0(LN(text_dense(SiLU(text))))
    GemmParams p = gp_text(c, c.Lt, w.d);
    p.seg[0] = GemmSeg{TS(c, text_out), w.w_td, dt, 1, 1};
    p.bias0 = w.b_td;
    p.ln = 1;
    set_film(c, p, w.f0, 1);
    p.out = ELT(c, li, tl);
    run_gemm(c, "enc.text_dense", p);
  }
  if (v_rows(h, w)) {
    // the fused bf16 EncoderLayer kernels read the values as rows [B*Lt, d] (attn_core.h): K and V as two launches of the
    // stacked [2d x d] weight's halves (this generic text path only runs with DHW_FUSE_TEXT=0 / unsupported text shapes)
    for (int half = 0; half < 2; ++half) {
      GemmParams p = gp_base(c, c.Lt, w.d);
      p.seg[0] = GemmSeg{ELT(c, li, tl), (const char*)w.w_kv1 + (size_t)half * w.d * w.d * h->es, w.d, 1, 0};
      p.bias0 = w.b_kv1 + half * w.d;
      if (half == 0) { p.posb = w.pb_k1; p.posb_cols = w.d; }
      p.out = half ? ELT(c, li, vt1) : ELT(c, li, k1);
      run_gemm(c, half ? "enc.v_text" : "enc.k_text", p);
    }
  } else {  // k1 = Wk(tl + PE), v1 = Wv(tl)   (values carry no PE: model.py:46)
    GemmParams p = gp_base(c, c.Lt, 2 * w.d);
    p.seg[0] = GemmSeg{ELT(c, li, tl), w.w_kv1, w.d, 1, 0};
    p.bias0 = w.b_kv1;
    p.posb = w.pb_k1;
    p.posb_cols = w.d;
    p.n_store = w.d;
    p.out = ELT(c, li, k1);
    p.vt = ELT(c, li, vt1);
    p.vt_lpad = h->lpadT;
    run_gemm(c, "enc.kv_text", p);
  }
  tap_text_kv(c, li, w, v_rows(h, w));
}

// parameters of the fused EncoderLayer kernels for layer n (x may be null when the tile is handed over in LDS)
EncLayerParams enc_params(Ctx& c, int li, const EncLayerW& w, const void* x, int Lk, int lpad, const int64_t* text,
                          void* pool) {
  dhw_handle* h = c.h;
  const int d = w.d;
  // text keys/values of this layer: per-call buffers, or step `plane_step` of the all-steps plane
  const char* k1p = (const char*)ELK(c, li, k1);
  const char* vt1p = (const char*)ELK(c, li, vt1);
  if (c.use_plane) {
    k1p += (size_t)c.plane_step * c.B * c.Lt * d * h->es;
    vt1p += (size_t)c.plane_step * c.B * (v_rows(h, w) ? c.Lt : h->lpadT) * d * h->es;
  }
  EncLayerParams q{};
  q.B = c.B; q.Lk = Lk; q.Lt = c.Lt; q.d = d; q.heads = w.heads;
  q.x = x;
  q.w_q1 = w.w_q1; q.w_d1 = w.w_d1; q.w_qkv2 = w.w_qkv2; q.w_d2 = w.w_d2; q.w_f1 = w.w_f1; q.w_f2 = w.w_f2;
  q.b_q1 = w.b_q1; q.b_d1 = w.b_d1; q.b_qkv2 = w.b_qkv2; q.b_d2 = w.b_d2; q.b_f1 = w.b_f1; q.b_f2 = w.b_f2;
  q.pb_q1 = w.pb_q1; q.pb_qk2 = w.pb_qk2;
  q.film = c.film; q.film_bs = c.film_bs; q.film_tot = h->film_tot; q.f1 = w.f1; q.f2 = w.f2; q.f3 = w.f3;
  q.k1 = k1p; q.vt1 = vt1p; q.lpadT = h->lpadT; q.text = text;
  q.x2 = ELB(c, li, x2); q.qk2 = ELB(c, li, qk2); q.vt2 = ELB(c, li, vt2); q.lpadX = lpad;
  q.out = ELB(c, li, out); q.pool = pool;
  q.lens = c.lens; q.lsh = level_shift(c.L, Lk);
  q.store_a = store_policy_of(h->store_policy, 1); q.store_bc = store_policy_of(h->store_policy, 2);
  return q;
}

// skip_a: this layer's enc_a half was already evaluated by the previous launch (EncChain); chain: what this layer's
// enc_bc launch continues with (or null)
static void enc_layer(Ctx& c, int li, const EncLayerW& w, const void* x, int Lk, int lpad, const int64_t* text,
               void* pool, bool skip_a = false, const EncChain* chain = nullptr, int bm_min = 0) {
  dhw_handle* h = c.h;
  const int d = w.d;
  const char* k1p = (const char*)ELK(c, li, k1);
  const char* vt1p = (const char*)ELK(c, li, vt1);
  if (c.use_plane) {
    k1p += (size_t)c.plane_step * c.B * c.Lt * d * h->es;
    vt1p += (size_t)c.plane_step * c.B * (v_rows(h, w) ? c.Lt : h->lpadT) * d * h->es;
  }
  if (h->fuse && enclayer_supported(h->prec, d, w.heads)) {
    EncLayerParams q = enc_params(c, li, w, x, Lk, lpad, text, pool);
    q.bm_min = bm_min;
    const double rows = (double)c.B * Lk, dd = d;
    if (c.rec) {
      const bool chained = chain && chain->mode;
      if (h->prec != PREC_BF16) { c.rec_fail = true; return; }
      if (!skip_a) {
        if (d == 256) rec_phase(c, PK_A256, c.L, nullptr, &q, nullptr);
        else c.rec_fail = true;
      }
      int kind = -1;
      if (d == 192 && !chained && skip_a) kind = PK_BC192;
      else if (d == 256 && chained && chain->mode == 2 && !skip_a && bm_min == 32 && !(Lk & 1)) kind = PK_BC256_N2;
      else if (d == 384 && chained && chain->mode == 1 && skip_a) kind = PK_BC384_N1;
      else if (d == 384 && !chained && skip_a) kind = PK_BC384;
      if (kind < 0) { c.rec_fail = true; return; }
      rec_phase(c, kind, c.L, nullptr, &q, chained ? chain : nullptr);
      return;
    }
    for (int which = skip_a ? 1 : 0; which < 2 && !c.err; ++which) {
      double fl = which == 0 ? 2.0 * rows * dd * dd * 5 + 4.0 * rows * c.Lt * dd
                             : 2.0 * rows * dd * dd * 5 + 4.0 * rows * Lk * dd;
      double by = (which == 0 ? rows * dd * 5 : rows * dd * (5 + (pool ? 0.5 : 0.0))) * h->es + 5.0 * dd * dd * h->es;
      const EncChain* ch = which == 1 ? chain : nullptr;
      if (ch && ch->mode) {   // + the chained layer's enc_a (+ att_dense)
        const double r2 = (double)c.B * ch->a.Lk, d2 = ch->a.d;
        fl += 2.0 * r2 * d2 * d2 * 5 + 4.0 * r2 * c.Lt * d2 + (ch->mode == 2 ? 2.0 * r2 * dd * d2 : 0.0);
        by += r2 * d2 * 5 * h->es + 5.0 * d2 * d2 * h->es;
      }
      Launch l(h, c.st, which == 0 ? "enc.fused_a" : (ch && ch->mode ? "enc.fused_bc+a" : "enc.fused_bc"), fl, by);
      hipError_t e = q.lens ? launch_enclayer_ragged(h->prec, q, which, c.st, ch)
                     : h->store_policy != DHW_STORE_DEFAULT ? launch_enclayer_policy(h->prec, q, which, c.st, ch) : launch_enclayer(h->prec, q, which, c.st, ch);
      if (e != hipSuccess) c.err = fail(h, DHW_ERR_HIP, "enclayer %s/%d: %s", h->el_name[li].c_str(), which, hipGetErrorString(e));
    }
    tap(c, tap_el(li, 1), ELB(c, li, x2), Lk, d);
    tap(c, tap_el(li, 0), ELB(c, li, out), Lk, d);
    if (pool && li < 2) tap(c, li == 0 ? TAP_POOL3 : TAP_POOL5, pool, Lk / 2, d);
    return;
  }
  if (c.rec) { c.rec_fail = true; return; }
  {  // q1 = Wq(x + PE)
    GemmParams p = gp_stroke(c, Lk, d);
    p.seg[0] = GemmSeg{x, w.w_q1, d, 1, 0};
    p.bias0 = w.b_q1;
    p.posb = w.pb_q1;
    p.posb_cols = d;
    p.out = ELB(c, li, q1);
    run_gemm(c, "enc.q_cross", p);
  }
  {
    AttnParams a{};
    a.Q = ELB(c, li, q1); a.ldq = d;
    a.K = k1p; a.ldk = d; a.koff = 0;
    a.Vt = vt1p; a.lpad = h->lpadT;
    a.text = text; a.ldt = c.Lt;
    a.out = ELB(c, li, a1); a.ldo = d;
    a.B = c.B; a.H = w.heads; a.D = d / w.heads; a.Lq = Lk; a.Lk = c.Lt;
    a.lens = c.lens; a.lsh = level_shift(c.L, Lk);   // (ragged: this sample's query rows; the keys are the text's)
    run_attn(c, "attn.cross", a);
  }
  {  // x2 = FiLM1(LN(dense(a1))) + x
    GemmParams p = gp_stroke(c, Lk, d);
    p.seg[0] = GemmSeg{ELB(c, li, a1), w.w_d1, d, 1, 0};
    p.bias0 = w.b_d1;
    p.ln = 1;
    set_film(c, p, w.f1, 1);
    p.res2 = x;
    p.out = ELB(c, li, x2);
    run_gemm(c, "enc.dense_cross", p);
  }
  {  // q2,k2 = W(x2 + PE), v2 = Wv x2
    GemmParams p = gp_stroke(c, Lk, 3 * d);
    p.seg[0] = GemmSeg{ELB(c, li, x2), w.w_qkv2, d, 1, 0};
    p.bias0 = w.b_qkv2;
    p.posb = w.pb_qk2;
    p.posb_cols = 2 * d;
    p.n_store = 2 * d;
    p.out = ELB(c, li, qk2);
    p.vt = ELB(c, li, vt2);
    p.vt_lpad = lpad;
    run_gemm(c, "enc.qkv_self", p);
  }
  {
    AttnParams a{};
    a.Q = ELB(c, li, qk2); a.ldq = 2 * d;
    a.K = ELB(c, li, qk2); a.ldk = 2 * d; a.koff = d;
    a.Vt = ELB(c, li, vt2); a.lpad = lpad;
    a.text = nullptr;
    a.out = ELB(c, li, a2); a.ldo = d;
    a.B = c.B; a.H = w.heads; a.D = d / w.heads; a.Lq = Lk; a.Lk = Lk;
    a.lens = c.lens; a.lsh = level_shift(c.L, Lk); a.lens_keys = 1;   // (ragged: this sample's rows are its keys)
    run_attn(c, "attn.self", a);
  }
  {  // x3 = FiLM2(LN(x2 + dense(a2)))
    GemmParams p = gp_stroke(c, Lk, d);
    p.seg[0] = GemmSeg{ELB(c, li, a2), w.w_d2, d, 1, 0};
    p.bias0 = w.b_d2;
    p.res1 = ELB(c, li, x2);
    p.ln = 1;
    set_film(c, p, w.f2, 1);
    p.out = ELB(c, li, x3);
    run_gemm(c, "enc.dense_self", p);
  }
  {  // f = SiLU(W1 SiLU(x3) + b1)
    GemmParams p = gp_stroke(c, Lk, 2 * d);
    p.seg[0] = GemmSeg{ELB(c, li, x3), w.w_f1, d, 1, 1};
    p.bias0 = w.b_f1;
    p.silu_out = 1;
    p.out = ELB(c, li, f);
    run_gemm(c, "enc.ffn1", p);
  }
  {  // out = FiLM3(LN(W2 f + b2 + x3))
    GemmParams p = gp_stroke(c, Lk, d);
    p.seg[0] = GemmSeg{ELB(c, li, f), w.w_f2, 2 * d, 1, 0};
    p.bias0 = w.b_f2;
    p.res1 = ELB(c, li, x3);
    p.ln = 1;
    set_film(c, p, w.f3, 1);
    p.out = ELB(c, li, out);
    p.pool = pool;
    run_gemm(c, "enc.ffn2", p);
  }
  tap(c, tap_el(li, 1), ELB(c, li, x2), Lk, d);
  tap(c, tap_el(li, 2), ELB(c, li, x3), Lk, d);
  tap(c, tap_el(li, 0), ELB(c, li, out), Lk, d);
  if (pool && li < 2) tap(c, li == 0 ? TAP_POOL3 : TAP_POOL5, pool, Lk / 2, d);
}

// sigma-independent prefix of TextStyleEncoder (text_style.py:92-97 up to the LayerNorms; Dropout is identity in eval)
void text_style_static(Ctx& c, const int64_t* text, const float* style) {
  dhw_handle* h = c.h;
  const int c2 = h->dims.c2, dt = 2 * c2;
  RUN_SMALL(c, "cast.style", launch_cast(h->prec, style, (long)c.B * c.S5 * STYLE_CH, WS(c, sty_in), c.st));
  {
    GemmParams p = gp_base(c, c.S5, 4 * c2);
    p.seg[0] = GemmSeg{WS(c, sty_in), h->w_sf1, STYLE_CH, 1, 1};
    p.bias0 = h->b_sf1;
    p.silu_out = 1;
    p.out = WS(c, sty_h);
    run_gemm(c, "style.ffn1", p);
  }
  {
    GemmParams p = gp_base(c, c.S5, dt);
    p.seg[0] = GemmSeg{WS(c, sty_h), h->w_sf3, 4 * c2, 1, 0};
    p.bias0 = h->b_sf3;
    p.ln = 1;
    p.out = WS(c, sty_n);
    run_gemm(c, "style.ffn2_ln", p);
  }
  RUN_SMALL(c, "embed_ln", launch_embed_ln(h->prec, text, c.B * c.Lt, h->emb, dt, true_width(h, dt), VOCAB, WS(c, t_n), c.st));
}

// sigma-dependent part of TextStyleEncoder (text_style.py:94-104) + the per-layer text projections
void text_style_dynamic(Ctx& c) {
  dhw_handle* h = c.h;
  const int c2 = h->dims.c2, dt = 2 * c2;
  const float* g = c.film;
  const float* bt = c.film + h->film_tot;
  const int in_B = c.in_B ? c.in_B : c.B;
  if (h->fuse && h->fuse_text && textside_supported(h->prec, c.Lt, c.S5, dt)) {
    // one workgroup per (step, prompt) pair, every intermediate in LDS (textside.hip)
    TextStyleParams q{};
    q.n = c.B; q.in_B = in_B; q.Lt = c.Lt; q.S5 = c.S5;
    q.sty_n = WS(c, sty_n); q.t_n = WS(c, t_n);
    q.film = c.film; q.film_bs = c.film_bs; q.film_div = c.film_div; q.film_tot = h->film_tot;
    q.f1 = h->f_ts1; q.f2 = h->f_ts2; q.f3 = h->f_ts3; q.f4 = h->f_ts4;
    q.w_q8 = h->w_q8; q.w_kv8 = h->w_kv8; q.w_d8 = h->w_d8; q.w_tf1 = h->w_tf1; q.w_tf3 = h->w_tf3;
    q.b_q8 = h->b_q8; q.b_kv8 = h->b_kv8; q.b_d8 = h->b_d8; q.b_tf1 = h->b_tf1; q.b_tf3 = h->b_tf3;
    q.text_out = TS(c, text_out);
    // plane reuse: only the all-steps launches of the sampling loop carry the flag; per-step launches, dhw_forward and the
    // generic path below always evaluate
    const unsigned* skip = c.planeT ? c.plane_skip : nullptr;
    const int pcall = skip ? c.plane_call : -1;
    q.skip = skip;
    if (!c.err) {
      const double n = c.B, ddt = dt;
      Launch l(h, c.st, "ts.fused", n * (2.0 * c.S5 * ddt * 2 * ddt + 2.0 * c.Lt * ddt * ddt * 2 + 4.0 * c.Lt * c.S5 * ddt + 2.0 * c.Lt * ddt * 2 * ddt * 2),
               n * c.Lt * ddt * h->es + (double)in_B * (c.S5 + c.Lt) * ddt * h->es + 8.0 * ddt * ddt * h->es, pcall);
      hipError_t e = launch_text_style(h->prec, q, c.st);
      if (e != hipSuccess) c.err = fail(h, DHW_ERR_HIP, "text_style fused: %s", hipGetErrorString(e));
    }
    if (!c.planeT) tap(c, TAP_TS, TS(c, text_out), c.Lt, dt);
    for (size_t i = 0; i < h->el.size() && !c.err; ++i) {
      const EncLayerW& w = h->el[i];
      TextLayerParams t{};
      t.n = c.B; t.Lt = c.Lt; t.d = w.d;
      t.text_out = TS(c, text_out);
      t.w_td = w.w_td; t.b_td = w.b_td;
      t.film = c.film; t.film_bs = c.film_bs; t.film_div = c.film_div; t.film_tot = h->film_tot; t.f0 = w.f0;
      t.w_kv = w.w_kv1; t.b_kv = w.b_kv1; t.pb_k1 = w.pb_k1;
      t.k1 = ELT(c, (int)i, k1); t.vt1 = ELT(c, (int)i, vt1); t.lpadT = h->lpadT;
      if (c.err) break;
      t.pairs = h->text_pairs;
      t.skip = skip;
      const double n = c.B, dd = w.d;
      Launch l(h, c.st, "enc.text_fused", n * c.Lt * (2.0 * dt * dd + 4.0 * dd * dd), n * c.Lt * (dt + 2.0 * dd) * h->es + (dt * dd + 2.0 * dd * dd) * h->es, pcall);
      hipError_t e = launch_text_layer(h->prec, t, c.st);
      if (e != hipSuccess) c.err = fail(h, DHW_ERR_HIP, "text layer %s: %s", h->el_name[i].c_str(), hipGetErrorString(e));
      tap_text_kv(c, (int)i, w, true);   // (text_layer_kernel copies v1 out as rows)
    }
    return;
  }
  RUN_SMALL(c, "film.style", launch_film_apply(h->prec, WS(c, sty_n), in_B, c.B, c.S5, dt, g + h->f_ts1, bt + h->f_ts1, c.film_bs, c.film_div, TS(c, s1), c.st));
  RUN_SMALL(c, "film.text", launch_film_apply(h->prec, WS(c, t_n), in_B, c.B, c.Lt, dt, g + h->f_ts2, bt + h->f_ts2, c.film_bs, c.film_div, TS(c, t1), c.st));
  {
    GemmParams p = gp_text(c, c.Lt, dt);
    p.seg[0] = GemmSeg{TS(c, t1), h->w_q8, dt, 1, 0};
    p.bias0 = h->b_q8;
    p.out = TS(c, q8);
    run_gemm(c, "ts.q", p);
  }
  {
    GemmParams p = gp_base(c, c.S5, 2 * dt);
    p.seg[0] = GemmSeg{TS(c, s1), h->w_kv8, dt, 1, 0};
    p.bias0 = h->b_kv8;
    p.n_store = dt;
    p.out = TS(c, k8);
    p.vt = TS(c, vt8);
    p.vt_lpad = h->lpadS;
    run_gemm(c, "ts.kv", p);
  }
  {
    AttnParams a{};
    a.Q = TS(c, q8); a.ldq = dt;
    a.K = TS(c, k8); a.ldk = dt; a.koff = 0;
    a.Vt = TS(c, vt8); a.lpad = h->lpadS;
    a.out = TS(c, a8); a.ldo = dt;
    a.B = c.B; a.H = 8; a.D = dt / 8; a.Lq = c.Lt; a.Lk = c.S5;
    run_attn(c, "attn.text_style", a);
  }
  {
    GemmParams p = gp_text(c, c.Lt, dt);
    p.seg[0] = GemmSeg{TS(c, a8), h->w_d8, dt, 1, 0};
    p.bias0 = h->b_d8;
    p.res1 = TS(c, t1);
    p.ln = 1;
    set_film(c, p, h->f_ts3, 1);
    p.out = TS(c, t2);
    run_gemm(c, "ts.dense", p);
  }
  {
    GemmParams p = gp_text(c, c.Lt, 2 * dt);
    p.seg[0] = GemmSeg{TS(c, t2), h->w_tf1, dt, 1, 1};
    p.bias0 = h->b_tf1;
    p.silu_out = 1;
    p.out = TS(c, tf_h);
    run_gemm(c, "ts.ffn1", p);
  }
  {
    GemmParams p = gp_text(c, c.Lt, dt);
    p.seg[0] = GemmSeg{TS(c, tf_h), h->w_tf3, 2 * dt, 1, 0};
    p.bias0 = h->b_tf3;
    p.ln = 1;
    set_film(c, p, h->f_ts4, 1);
    p.out = TS(c, text_out);
    run_gemm(c, "ts.ffn2", p);
  }
  if (!c.planeT) {
    tap(c, TAP_TS_STYLE, TS(c, s1), c.S5, dt);
    tap(c, TAP_TS_T2, TS(c, t2), c.Lt, dt);
    tap(c, TAP_TS, TS(c, text_out), c.Lt, dt);
  }
  for (size_t i = 0; i < h->el.size(); ++i) enc_layer_text(c, (int)i, h->el[i]);
}

// the stroke path of DiffusionModel.forward (model.py:139-182); the heads are launched by the caller
void stroke_path(Ctx& c, const float* strokes, const int64_t* text) {
  dhw_handle* h = c.h;
  const dhw_dims& d = h->dims;
  const int L = c.L, dt = 2 * d.c2;
  const bool fin = c.fuse_input && h->fuse;
  if (!fin) {
    RUN_SMALL(c, "input_dense", launch_input_dense(h->prec, strokes, (long)c.B * L, h->in_w, h->in_b, d.c1, WS(c, x0), c.st));
    tap(c, TAP_INPUT_DENSE, WS(c, x0), L, d.c1);
  }
  conv_block(c, CB_ENC1, h->enc1, WS(c, x0), L, CBB(c, CB_ENC1, out), false, WS(c, enc1_pool), fin ? strokes : nullptr);
  // Everything between two self-attentions is row-local: enc2 / enc4 continue into the first half of enc3 / enc5,
  // enc5's second half into AvgPool + att_dense + the first attention layer's first half, and every attention layer's
  // second half into the next layer's first half.
  const bool chain_ok = h->fuse && h->chain && h->prec == PREC_BF16;
  const int nl = d.num_layers;
  bool a3 = false, a5 = false;
  // enc2 / enc4 can continue into enc3.a / enc5.a the same way (bit 0 / bit 1), but the ConvBlock's row tiling (62 / 46 rows)
  // is a worse fit for the layer than its own: r1 measured 23.22 ms (off) / 23.21 (enc3) / 23.40 (enc5, both); r3, after the kernels
  // changed: 19.54 (off) / 19.40 (enc3: bit 0) / 19.62 (enc5: bit 1) / 19.45 (both), three alternating runs each -> enc3 only
  // r5: with enc4 on the asymmetric 32-row tiles (B = 64 at L / 4 = 122: the layer's own tiling) the enc5 chain wins, 18.02 -> 17.89 ms: the default
  // (no DHW_CHAIN_CONV) takes bit 1 exactly there (convblock_chain_auto); an explicit DHW_CHAIN_CONV forces / forbids it for any tiling
  static const bool conv_chain_env = getenv("DHW_CHAIN_CONV") != nullptr;
  static const int conv_chain = conv_chain_env ? atoi(getenv("DHW_CHAIN_CONV")) : 3;
  {
    EncChain ch{};
    if (chain_ok && (conv_chain & 1)) { ch.mode = 1; ch.a = enc_params(c, 0, h->el[0], nullptr, L / 2, h->lpadX[0], text, nullptr); }
    conv_block(c, CB_ENC2, h->enc2, WS(c, enc1_pool), L / 2, CBB(c, CB_ENC2, out), false, nullptr, nullptr, nullptr, ch.mode ? &ch : nullptr, &a3);
  }
  enc_layer(c, 0, h->el[0], CBB(c, CB_ENC2, out), L / 2, h->lpadX[0], text, WS(c, enc3_pool), a3);
  {
    EncChain ch{};
    // (record mode: the persistent step kernel has enc4 and enc5.a as two phases)
    if (chain_ok && (conv_chain & 2) && !c.rec) { ch.mode = 1; ch.a = enc_params(c, 1, h->el[1], nullptr, L / 4, h->lpadX[1], text, nullptr); }
    conv_block(c, CB_ENC4, h->enc4, WS(c, enc3_pool), L / 4, CBB(c, CB_ENC4, out), false, nullptr, nullptr, nullptr, ch.mode ? &ch : nullptr, &a5, !conv_chain_env);
  }
  EncChain ch5{};
  if (chain_ok && nl > 0 && enclayer_supported(h->prec, dt, h->el[2].heads) && enclayer_chain_supported(h->prec, d.c3, c.B, L / 4, 2, dt)) {
    ch5.mode = 2;
    ch5.a = enc_params(c, 2, h->el[2], nullptr, L / 8, h->lpadX[2], text, nullptr);
    ch5.w_dense = h->w_attd; ch5.b_dense = h->b_attd; ch5.dense_out = WS(c, att_dense);
  }
  enc_layer(c, 1, h->el[1], CBB(c, CB_ENC4, out), L / 4, h->lpadX[1], text, WS(c, enc5_pool), a5, ch5.mode ? &ch5 : nullptr,
            ch5.mode ? 32 : 0);
  if (!ch5.mode) {
    GemmParams p = gp_base(c, L / 8, dt);
    p.seg[0] = GemmSeg{WS(c, enc5_pool), h->w_attd, d.c3, 1, 0};
    p.bias0 = h->b_attd;
    p.out = WS(c, att_dense);
    p.lens = c.lens; p.lsh = 3;
    run_gemm(c, "att_dense", p);
  }
  tap(c, TAP_ATT_DENSE, WS(c, att_dense), L / 8, dt);
  const void* x = WS(c, att_dense);
  bool a_done = ch5.mode != 0;   // this layer's first half was evaluated by the previous launch
  for (int i = 0; i < nl; ++i) {
    EncChain chn{};
    if (chain_ok && i + 1 < nl && enclayer_chain_supported(h->prec, dt, c.B, L / 8, 1, dt)) {
      chn.mode = 1;
      chn.a = enc_params(c, 3 + i, h->el[3 + i], nullptr, L / 8, h->lpadX[2], text, nullptr);
    }
    enc_layer(c, 2 + i, h->el[2 + i], x, L / 8, h->lpadX[2], text, nullptr, a_done, chn.mode ? &chn : nullptr);
    a_done = chn.mode != 0;
    x = ELB(c, 2 + i, out);
  }
  // decoder: x = Upsample(previous) + skip_conv(encoder output of the same resolution), then the ConvBlock (model.py:169-175)
  struct UP { int tap; const void* skip_in; void* w; float* b; int cin, cout, L; const void* low; int cb; };
  const UP ups[3] = {
      {TAP_UP3, ELB(c, 1, out), h->w_sk3, h->b_sk3, d.c3, dt, L / 4, x, CB_DEC3},
      {TAP_UP2, ELB(c, 0, out), h->w_sk2, h->b_sk2, d.c2, d.c3, L / 2, CBB(c, CB_DEC3, out), CB_DEC2},
      {TAP_UP1, CBB(c, CB_ENC1, out), h->w_sk1, h->b_sk1, d.c1, d.c2, L, CBB(c, CB_DEC2, out), CB_DEC1}};
  const ConvBlockW* decs[3] = {&h->dec3, &h->dec2, &h->dec1};
  const bool fup = h->fuse && h->fuse_up && h->prec == PREC_BF16;
  for (int i = 0; i < 3; ++i) {
    const UP& u = ups[i];
    if (fup) {   // the decoder block evaluates upsample(x) + skip_conv(h) while staging its input
      const UpIn in{u.skip_in, u.w, u.b, u.cin, u.low};
      h->taps[u.tap].set = false;
      conv_block(c, u.cb, *decs[i], nullptr, u.L, CBB(c, u.cb, out), i == 2, nullptr, nullptr, &in);
      continue;
    }
    void* xd = need(c, c.ws->xd[i], "xd");
    GemmParams p = gp_base(c, u.L, u.cout);   // upsample(x) + skip_conv(h)  (model.py:169-175)
    p.seg[0] = GemmSeg{u.skip_in, u.w, u.cin, 3, 0};
    p.bias0 = u.b;
    p.res2 = u.low;
    p.res2_half = 1;
    p.out = xd;
    p.lens = c.lens; p.lsh = level_shift(c.L, u.L);
    run_gemm(c, "skip_conv_up", p);
    tap(c, u.tap, xd, u.L, u.cout);
    conv_block(c, u.cb, *decs[i], xd, u.L, CBB(c, u.cb, out), i == 2, nullptr);
  }
}

int launch_heads_for(Ctx& c, HeadsParams hp) {
  dhw_handle* h = c.h;
  hp.x = (const float*)CBB(c, CB_DEC1, out);
  hp.rows = (long)c.B * c.L;
  hp.C = h->dims.c1;
  hp.w_out = h->out_w; hp.b_out = h->out_b; hp.w_pen = h->pen_w; hp.b_pen = h->pen_b;
  hp.L = c.L;
  RUN_SMALL(c, "heads_step", launch_heads(hp, c.st));
  return c.err;
}
