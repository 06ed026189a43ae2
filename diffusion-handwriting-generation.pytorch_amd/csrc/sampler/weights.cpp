// sampler/weights.cpp — the state_dict inventory (mirrors spec.py), the embedding of narrower models into the kernels'
// physical widths, and dhw_finalize: weight repacking into MFMA-fragment order, the sigma-FiLM layout, PE·W position-bias tables.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handle.h"

// ---------------------------------------------------------------- state_dict inventory (mirrors spec.py)
static void add_linear(std::vector<KeySpec>& s, const std::string& n, int cin, int cout) {
  s.push_back({n + ".weight", {cout, cin}});
  s.push_back({n + ".bias", {cout}});
}
static void add_conv(std::vector<KeySpec>& s, const std::string& n, int cin, int cout) {
  s.push_back({n + ".weight", {cout, cin, 3}});
  s.push_back({n + ".bias", {cout}});
}
static void add_affine(std::vector<KeySpec>& s, const std::string& n, int c) {
  add_linear(s, n + ".gamma_emb", SIG, c);
  add_linear(s, n + ".beta_emb", SIG, c);
}
static void add_convblock(std::vector<KeySpec>& s, const std::string& n, int cin, int cout) {
  add_affine(s, n + ".affine1", cout / 2);
  add_affine(s, n + ".affine2", cout);
  add_affine(s, n + ".affine3", cout);
  add_conv(s, n + ".conv_skip", cin, cout);
  add_conv(s, n + ".conv1", cin, cout / 2);
  add_conv(s, n + ".conv2", cout / 2, cout);
  add_linear(s, n + ".fc", cout, cout);
}
static void add_mha(std::vector<KeySpec>& s, const std::string& n, int d) {
  for (const char* w : {".wq", ".wk", ".wv", ".dense"}) add_linear(s, n + w, d, d);
}
static void add_enclayer(std::vector<KeySpec>& s, const std::string& n, int dinp, int d) {
  add_linear(s, n + ".text_dense", dinp, d);
  add_linear(s, n + ".ffn.1", d, 2 * d);
  add_linear(s, n + ".ffn.3", 2 * d, d);
  add_mha(s, n + ".mha", d);
  add_mha(s, n + ".mha2", d);
  for (int k = 0; k < 4; ++k) add_affine(s, n + ".affine" + std::to_string(k), d);
}
std::vector<KeySpec> build_spec(int nl, int c1, int c2, int c3) {
  std::vector<KeySpec> s;
  const int dt = 2 * c2;
  add_linear(s, "input_dense", 2, c1);
  add_linear(s, "sigma_ffn.1", 1, SIG_HID);
  add_linear(s, "sigma_ffn.3", SIG_HID, c1 / 4);
  add_convblock(s, "enc1", c1, c1);
  add_convblock(s, "enc2", c1, c2);
  add_enclayer(s, "enc3", dt, c2);
  add_convblock(s, "enc4", c2, c3);
  add_enclayer(s, "enc5", dt, c3);
  add_conv(s, "skip_conv1", c1, c2);
  add_conv(s, "skip_conv2", c2, c3);
  add_conv(s, "skip_conv3", c3, dt);
  const std::string t = "text_style_model";
  s.push_back({t + ".emb.weight", {VOCAB, dt}});
  add_linear(s, t + ".style_ffn.1", STYLE_CH, 4 * c2);
  add_linear(s, t + ".style_ffn.3", 4 * c2, dt);
  add_linear(s, t + ".text_ffn.1", dt, 2 * dt);
  add_linear(s, t + ".text_ffn.3", 2 * dt, dt);
  add_mha(s, t + ".mha", dt);
  for (int k = 1; k <= 4; ++k) add_affine(s, t + ".affine" + std::to_string(k), dt);
  add_linear(s, "att_dense", 2 * c1, dt);
  for (int i = 0; i < nl; ++i) add_enclayer(s, "att_layers." + std::to_string(i), dt, dt);
  add_convblock(s, "dec3", dt, c3);
  add_convblock(s, "dec2", c3, c2);
  add_convblock(s, "dec1", c2, c1);
  add_linear(s, "output_dense", c1, 2);
  add_linear(s, "pen_lifts_dense.0", c1, 1);
  return s;
}

// A weight by state_dict key (finalize-time only): the padded copy on a padded handle.  A miss is a programming error
// (WeightStore::find): it is recorded, dhw_finalize then returns DHW_ERR_INTERNAL and a short all-zero tensor comes back, so every
// reader checks before it indexes: the upload helpers refuse once lookup_fail is set, conv_w below checks the size — nothing throws.
static const std::vector<float>& W(dhw_handle* h, const std::string& key) {
  bool first = false;
  const int i = h->store.find(key, &first);
  if (first) fail(h, DHW_ERR_INTERNAL, "internal: the packing code asked for an unknown weight '%s'", key.c_str());
  return i < 0 ? WeightStore::zeros() : (h->padded ? h->phys_w : h->store.host_w)[i];
}
static int film_offset(dhw_handle* h, const std::string& name) {
  auto it = h->film_off.find(name);
  if (it == h->film_off.end()) {
    if (!h->store.lookup_fail) fail(h, DHW_ERR_INTERNAL, "internal: no FiLM layer named '%s'", name.c_str());
    h->store.lookup_fail = true;
    return 0;
  }
  return it->second;
}

static int upload_f32(dhw_handle* h, const std::vector<float>& v, float** out) {
  if (h->store.lookup_fail) return DHW_ERR_INTERNAL;
  ARENACK(h, upload_f32(v, out));
  return 0;
}
// a row-major weight matrix Wf[N][K] in MFMA-fragment order (host/convert.h pack_mfma), in the handle's element type
static int upload_packed(dhw_handle* h, const std::vector<float>& wf, int N, int K, void** out) {
  if (h->store.lookup_fail) return DHW_ERR_INTERNAL;
  if (N % 16 || K % 32 || (size_t)N * K != wf.size()) return fail(h, DHW_ERR_INTERNAL, "pack: bad shape %d x %d", N, K);
  ARENACK(h, upload_packed(wf, N, K, h->prec != PREC_F32, out));
  return 0;
}
// Conv1d weight `key` [cout][cin][3] as its GEMM matrix (conv_flat); empty — which upload_packed refuses — when the tensor is not that size
static std::vector<float> conv_w(dhw_handle* h, const std::string& key, int cout, int cin) {
  const std::vector<float>& w = W(h, key);
  return w.size() == (size_t)cout * cin * 3 ? conv_flat(w, cout, cin) : std::vector<float>();
}
static std::vector<float> vcat(std::initializer_list<const std::vector<float>*> vs) {
  std::vector<float> r;
  for (auto v : vs) r.insert(r.end(), v->begin(), v->end());
  return r;
}

// Sinusoidal table PE[pos][dim] exactly as attention.py:15-23 evaluates it in fp32.
// (dim_true < dim: the model's width is below the kernels' physical one; the table keeps the row stride dim, the values of the
// dim_true-wide encoding sit in columns [0, dim_true) and the rest is zero — the tail padding of pad_weights)
static std::vector<float> pe_table(int n, int dim, float pos_factor, int dim_true = 0) {
  if (dim_true <= 0) dim_true = dim;
  const int half = dim_true / 2;
  const float negc = (float)(-(std::log(10000.0) / (half - 1)));
  std::vector<float> pe((size_t)n * dim);
  for (int j = 0; j < half; ++j) {
    const float f = expf((float)j * negc);
    for (int t = 0; t < n; ++t) {
      const float e = ((float)t * f) * pos_factor;
      pe[(size_t)t * dim + j] = sinf(e);
      pe[(size_t)t * dim + half + j] = cosf(e);
    }
  }
  return pe;
}
// posb[pos][n] = sum_k PE[pos][k] * Wm[n][k]   (Wm: [N][dim] row-major)
static std::vector<float> pe_times_w(const std::vector<float>& pe, int n, int dim, const std::vector<float>& wm, int N) {
  std::vector<float> r((size_t)n * N);
  for (int t = 0; t < n; ++t)
    for (int o = 0; o < N; ++o) {
      double a = 0;
      const float* p = &pe[(size_t)t * dim];
      const float* w = &wm[(size_t)o * dim];
      for (int k = 0; k < dim; ++k) a += (double)p[k] * (double)w[k];
      r[(size_t)t * N + o] = (float)a;
    }
  return r;
}

// ---------------------------------------------------------------- model widths below the kernels' (c2 < 192)
// The reference's constructor takes any c2 divisible by 12 (model.py:64-71: 3 heads at c2, 6 at 2*c2, 8 in the TextStyleEncoder,
// text_style.py:78).  The kernels are built for c2 = 192: head dims 64 and 48, LayerNorm widths 192 / 384.  A smaller model is
// EMBEDDED into those shapes: every c2-derived channel axis is zero padded at the tail (c2/2 -> 96, c2 -> 192, 2*c2 -> 384,
// 4*c2 -> 768) and the q / k / v projections' output axis (= the attention dense's input axis) head by head (head h's c2/3 or
// c2/4 channels at the front of its 64- or 48-wide slot).  With zero weights, biases and FiLM rows in the padding every padded
// channel stays exactly 0 through convolutions, SiLU, residuals, pooling and attention; what is left to handle is (1) LayerNorm:
// statistics over the true width, padding written as 0 (GemmParams::ln_n, embed_ln's n_true), (2) the attention's 1/sqrt(depth):
// the kernels scale by the physical head dim, so wq / its bias (and with them PE·Wq) carry sqrt(physical / true), (3) the
// positional encodings, evaluated for the true width (pe_table).  Such a handle runs the one-launch-per-GEMM path (fuse = false):
// the fused block kernels keep their compile-time LayerNorm widths.
int true_width(const dhw_handle* h, int n) {
  if (!h->padded) return n;
  const int c2 = h->ldims.c2;
  switch (n) {
    case 96: return c2 / 2;
    case 192: return c2;
    case 384: return 2 * c2;
    case 768: return 4 * c2;
    default: return n;   // c1 = 128 and c3 = 256 are fixed, so 32 / 64 / 128 / 256 / 512 are never c2-derived
  }
}

static bool ends_with(const std::string& s, const char* suf) {
  const size_t n = std::strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

static int pad_weights(dhw_handle* h) {
  h->phys_w.assign(h->store.spec.size(), {});
  for (size_t i = 0; i < h->store.spec.size(); ++i) {
    const KeySpec& lk = h->store.spec[i];
    const KeySpec& pk = h->pspec[i];
    const std::string& key = lk.key;
    if (lk.shape.size() != pk.shape.size() || lk.shape.size() > 3) return fail(h, DHW_ERR_ARG, "pad: rank of %s", key.c_str());
    // heads of the attention module this tensor belongs to (0 = not a q/k/v/dense tensor of an attention)
    int heads = 0;
    if (key.find(".mha") != std::string::npos)
      heads = key.compare(0, 4, "enc3") == 0 ? 3 : key.compare(0, 4, "enc5") == 0 ? 4 : key.compare(0, 10, "att_layers") == 0 ? 6 : 8;
    const bool is_dense = key.find(".dense.") != std::string::npos;
    const bool is_q = key.find(".wq.") != std::string::npos;
    int head_axis = -1;   // axis laid out head by head
    if (heads) head_axis = is_dense ? (ends_with(key, ".weight") ? 1 : -1) : 0;
    int64_t ls[3] = {1, 1, 1}, ps[3] = {1, 1, 1};
    for (size_t a = 0; a < lk.shape.size(); ++a) { ls[a] = lk.shape[a]; ps[a] = pk.shape[a]; }
    std::vector<int64_t> map[3];
    float qscale = 1.0f;
    for (int a = 0; a < 3; ++a) {
      map[a].resize(ls[a]);
      if (a == head_axis && ls[a] != ps[a]) {
        const int64_t dl = ls[a] / heads, dp = ps[a] / heads;
        if (dl * heads != ls[a] || dp * heads != ps[a] || dl > dp) return fail(h, DHW_ERR_ARG, "pad: head split of %s", key.c_str());
        for (int64_t j = 0; j < ls[a]; ++j) map[a][j] = (j / dl) * dp + j % dl;
        if (is_q) qscale = std::sqrt((float)dp / (float)dl);
      } else {
        if (ls[a] > ps[a]) return fail(h, DHW_ERR_ARG, "pad: %s is wider than its physical shape", key.c_str());
        for (int64_t j = 0; j < ls[a]; ++j) map[a][j] = j;
      }
    }
    const std::vector<float>& src = h->store.host_w[i];
    std::vector<float>& dst = h->phys_w[i];
    dst.assign((size_t)(ps[0] * ps[1] * ps[2]), 0.f);
    size_t o = 0;
    for (int64_t x = 0; x < ls[0]; ++x)
      for (int64_t y = 0; y < ls[1]; ++y)
        for (int64_t z = 0; z < ls[2]; ++z) dst[(size_t)((map[0][x] * ps[1] + map[1][y]) * ps[2] + map[2][z])] = src[o++] * qscale;
  }
  return 0;
}

static int pack_convblock(dhw_handle* h, const std::string& n, int cin, int cout, ConvBlockW& cb) {
  cb.cin = cin;
  cb.cout = cout;
  int rc;
  if ((rc = upload_packed(h, conv_w(h, n + ".conv1.weight", cout / 2, cin), cout / 2, 3 * cin, &cb.w_c1))) return rc;
  if ((rc = upload_packed(h, conv_w(h, n + ".conv2.weight", cout, cout / 2), cout, 3 * (cout / 2), &cb.w_c2))) return rc;
  if ((rc = upload_packed(h, W(h, n + ".fc.weight"), cout, cout, &cb.w_fc))) return rc;
  if ((rc = upload_packed(h, conv_w(h, n + ".conv_skip.weight", cout, cin), cout, 3 * cin, &cb.w_skip))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".conv1.bias"), &cb.b_c1))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".conv2.bias"), &cb.b_c2))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".fc.bias"), &cb.b_fc))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".conv_skip.bias"), &cb.b_skip))) return rc;
  cb.f1 = film_offset(h, n + ".affine1");
  cb.f2 = film_offset(h, n + ".affine2");
  cb.f3 = film_offset(h, n + ".affine3");
  return 0;
}

static int pack_enclayer(dhw_handle* h, const std::string& n, int d, int heads, float pf, int max_lk, EncLayerW& e) {
  e.d = d;
  e.heads = heads;
  e.pos_factor = pf;
  const int dt = 2 * h->dims.c2;
  int rc;
  auto& wq1 = W(h, n + ".mha.wq.weight");
  auto& wk1 = W(h, n + ".mha.wk.weight");
  auto& wv1 = W(h, n + ".mha.wv.weight");
  auto& wq2 = W(h, n + ".mha2.wq.weight");
  auto& wk2 = W(h, n + ".mha2.wk.weight");
  auto& wv2 = W(h, n + ".mha2.wv.weight");
  if ((rc = upload_packed(h, W(h, n + ".text_dense.weight"), d, dt, &e.w_td))) return rc;
  if ((rc = upload_packed(h, vcat({&wk1, &wv1}), 2 * d, d, &e.w_kv1))) return rc;
  if ((rc = upload_packed(h, wq1, d, d, &e.w_q1))) return rc;
  if ((rc = upload_packed(h, W(h, n + ".mha.dense.weight"), d, d, &e.w_d1))) return rc;
  if ((rc = upload_packed(h, vcat({&wq2, &wk2, &wv2}), 3 * d, d, &e.w_qkv2))) return rc;
  if ((rc = upload_packed(h, W(h, n + ".mha2.dense.weight"), d, d, &e.w_d2))) return rc;
  if ((rc = upload_packed(h, W(h, n + ".ffn.1.weight"), 2 * d, d, &e.w_f1))) return rc;
  if ((rc = upload_packed(h, W(h, n + ".ffn.3.weight"), d, 2 * d, &e.w_f2))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".text_dense.bias"), &e.b_td))) return rc;
  if ((rc = upload_f32(h, vcat({&W(h, n + ".mha.wk.bias"), &W(h, n + ".mha.wv.bias")}), &e.b_kv1))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".mha.wq.bias"), &e.b_q1))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".mha.dense.bias"), &e.b_d1))) return rc;
  if ((rc = upload_f32(h, vcat({&W(h, n + ".mha2.wq.bias"), &W(h, n + ".mha2.wk.bias"), &W(h, n + ".mha2.wv.bias")}), &e.b_qkv2))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".mha2.dense.bias"), &e.b_d2))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".ffn.1.bias"), &e.b_f1))) return rc;
  if ((rc = upload_f32(h, W(h, n + ".ffn.3.bias"), &e.b_f2))) return rc;
  // (x + PE)·W = x·W + PE·W: the PE term is a per-position bias table (model.py:40-50, attention.py:15-23)
  const auto pe_t = pe_table(h->dims.max_Lt + SLACK_ROWS, d, 1.0f, true_width(h, d));   // text_pe_gen: pos_factor 1 (model.py:22)
  const auto pe_x = pe_table(max_lk + SLACK_ROWS, d, pf, true_width(h, d));             // stroke_pe_gen
  if ((rc = upload_f32(h, pe_times_w(pe_t, h->dims.max_Lt + SLACK_ROWS, d, wk1, d), &e.pb_k1))) return rc;
  if ((rc = upload_f32(h, pe_times_w(pe_x, max_lk + SLACK_ROWS, d, wq1, d), &e.pb_q1))) return rc;
  if ((rc = upload_f32(h, pe_times_w(pe_x, max_lk + SLACK_ROWS, d, vcat({&wq2, &wk2}), 2 * d), &e.pb_qk2))) return rc;
  e.f0 = film_offset(h, n + ".affine0");
  e.f1 = film_offset(h, n + ".affine1");
  e.f2 = film_offset(h, n + ".affine2");
  e.f3 = film_offset(h, n + ".affine3");
  return 0;
}

void build_film_layout(dhw_handle* h) {
  int off = 0;
  for (const KeySpec& k : h->pspec) {
    const std::string suf = ".gamma_emb.weight";
    if (k.key.size() > suf.size() && k.key.compare(k.key.size() - suf.size(), suf.size(), suf) == 0) {
      h->film_off[k.key.substr(0, k.key.size() - suf.size())] = off;
      off += (int)k.shape[0];
    }
  }
  h->film_tot = off;
}

#define UPF(dst, key) if ((rc = upload_f32(h, W(h, key), &h->dst))) return rc
int finalize_impl(dhw_handle* h) {
  if (!h) return fail(nullptr, DHW_ERR_ARG, "null handle");
  if (h->packed) return 0;
  if (const int m = h->store.first_missing(); m >= 0) return fail(h, DHW_ERR_KEY, "missing key in state_dict: %s", h->store.spec[m].key.c_str());
  HIPCK(h, hipSetDevice(h->device));
  HIPCK(h, hipDeviceSynchronize());
  drop_graphs(h);   // device is idle here (synchronised above); the resident text plane goes with the graphs
  ++h->weights_gen;
  const dhw_dims& d = h->dims;
  const int c1 = d.c1, c2 = d.c2, c3 = d.c3, dt = 2 * c2;
  int rc;
  if (h->padded && (rc = pad_weights(h))) return rc;
  // (re-packing leaks the previous packed copies until destroy; weights are loaded once in practice)
  {  // FiLM: all gamma/beta projections concatenated -> [2*TOT, 32]
    std::vector<float> w((size_t)2 * h->film_tot * SIG), b((size_t)2 * h->film_tot);
    for (auto& kv : h->film_off) {
      const auto& gw = W(h, kv.first + ".gamma_emb.weight");
      const auto& gb = W(h, kv.first + ".gamma_emb.bias");
      const auto& bw = W(h, kv.first + ".beta_emb.weight");
      const auto& bb = W(h, kv.first + ".beta_emb.bias");
      std::copy(gw.begin(), gw.end(), w.begin() + (size_t)kv.second * SIG);
      std::copy(gb.begin(), gb.end(), b.begin() + kv.second);
      std::copy(bw.begin(), bw.end(), w.begin() + (size_t)(h->film_tot + kv.second) * SIG);
      std::copy(bb.begin(), bb.end(), b.begin() + h->film_tot + kv.second);
    }
    if ((rc = upload_f32(h, w, &h->d_film_w))) return rc;
    if ((rc = upload_f32(h, b, &h->d_film_b))) return rc;
  }
  UPF(sg_w1, "sigma_ffn.1.weight"); UPF(sg_b1, "sigma_ffn.1.bias"); UPF(sg_w2, "sigma_ffn.3.weight"); UPF(sg_b2, "sigma_ffn.3.bias");
  UPF(in_w, "input_dense.weight"); UPF(in_b, "input_dense.bias");
  UPF(out_w, "output_dense.weight"); UPF(out_b, "output_dense.bias");
  UPF(pen_w, "pen_lifts_dense.0.weight"); UPF(pen_b, "pen_lifts_dense.0.bias");
  UPF(emb, "text_style_model.emb.weight");
  const std::string t = "text_style_model";
  UPF(b_sf1, t + ".style_ffn.1.bias"); UPF(b_sf3, t + ".style_ffn.3.bias"); UPF(b_q8, t + ".mha.wq.bias");
  UPF(b_d8, t + ".mha.dense.bias"); UPF(b_tf1, t + ".text_ffn.1.bias"); UPF(b_tf3, t + ".text_ffn.3.bias");
  UPF(b_attd, "att_dense.bias"); UPF(b_sk1, "skip_conv1.bias"); UPF(b_sk2, "skip_conv2.bias"); UPF(b_sk3, "skip_conv3.bias");
  if ((rc = upload_f32(h, vcat({&W(h, t + ".mha.wk.bias"), &W(h, t + ".mha.wv.bias")}), &h->b_kv8))) return rc;
  if ((rc = upload_packed(h, W(h, t + ".style_ffn.1.weight"), 4 * c2, STYLE_CH, &h->w_sf1))) return rc;
  if ((rc = upload_packed(h, W(h, t + ".style_ffn.3.weight"), dt, 4 * c2, &h->w_sf3))) return rc;
  if ((rc = upload_packed(h, W(h, t + ".mha.wq.weight"), dt, dt, &h->w_q8))) return rc;
  if ((rc = upload_packed(h, vcat({&W(h, t + ".mha.wk.weight"), &W(h, t + ".mha.wv.weight")}), 2 * dt, dt, &h->w_kv8))) return rc;
  if ((rc = upload_packed(h, W(h, t + ".mha.dense.weight"), dt, dt, &h->w_d8))) return rc;
  if ((rc = upload_packed(h, W(h, t + ".text_ffn.1.weight"), 2 * dt, dt, &h->w_tf1))) return rc;
  if ((rc = upload_packed(h, W(h, t + ".text_ffn.3.weight"), dt, 2 * dt, &h->w_tf3))) return rc;
  if ((rc = upload_packed(h, W(h, "att_dense.weight"), dt, 2 * c1, &h->w_attd))) return rc;
  if ((rc = upload_packed(h, conv_w(h, "skip_conv1.weight", c2, c1), c2, 3 * c1, &h->w_sk1))) return rc;
  if ((rc = upload_packed(h, conv_w(h, "skip_conv2.weight", c3, c2), c3, 3 * c2, &h->w_sk2))) return rc;
  if ((rc = upload_packed(h, conv_w(h, "skip_conv3.weight", dt, c3), dt, 3 * c3, &h->w_sk3))) return rc;
  h->f_ts1 = film_offset(h, t + ".affine1");
  h->f_ts2 = film_offset(h, t + ".affine2");
  h->f_ts3 = film_offset(h, t + ".affine3");
  h->f_ts4 = film_offset(h, t + ".affine4");
  if ((rc = pack_convblock(h, "enc1", c1, c1, h->enc1))) return rc;
  if ((rc = pack_convblock(h, "enc2", c1, c2, h->enc2))) return rc;
  if ((rc = pack_convblock(h, "enc4", c2, c3, h->enc4))) return rc;
  if ((rc = pack_convblock(h, "dec3", dt, c3, h->dec3))) return rc;
  if ((rc = pack_convblock(h, "dec2", c3, c2, h->dec2))) return rc;
  if ((rc = pack_convblock(h, "dec1", c2, c1, h->dec1))) return rc;
  h->el.assign(2 + d.num_layers, EncLayerW{});
  if ((rc = pack_enclayer(h, "enc3", c2, 3, 4.0f, d.max_L / 2, h->el[0]))) return rc;   // model.py:88
  if ((rc = pack_enclayer(h, "enc5", c3, 4, 2.0f, d.max_L / 4, h->el[1]))) return rc;   // model.py:90
  for (int i = 0; i < d.num_layers; ++i)
    if ((rc = pack_enclayer(h, "att_layers." + std::to_string(i), dt, 6, 1.0f, d.max_L / 8, h->el[2 + i]))) return rc;   // model.py:104-109
  HIPCK(h, hipDeviceSynchronize());
  if (h->store.lookup_fail) return DHW_ERR_INTERNAL;   // (message set by W / film_offset)
  h->packed = true;
  for (auto& kv : h->film_T) kv.second.ready = false;
  return 0;
}

#undef UPF
