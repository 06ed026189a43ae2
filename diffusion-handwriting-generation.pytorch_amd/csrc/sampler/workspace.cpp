// sampler/workspace.cpp — device memory of a handle: the activation workspaces, the all-steps text plane, the shared staging
// buffers, the names dhw_debug_read resolves, and the teardown.
#include "handle.h"

int dev_alloc(dhw_handle* h, void** p, size_t bytes, bool zero) {
  ARENACK(h, alloc(p, bytes, zero));
  return 0;
}

int ensure_scratch(dhw_handle* h) {
  dhw_handle::DenoiseScratch& s = h->scratch;
  if (s.x) return 0;
  const size_t cap = (size_t)h->dims.max_B * h->dims.max_L;
  int rc;
  if ((rc = dev_alloc(h, (void**)&s.w, cap * 2 * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&s.eps, cap * 2 * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&s.pen, cap * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&s.sigma, (size_t)h->dims.max_B * 4))) return rc;
  return dev_alloc(h, (void**)&s.x, cap * 2 * 4);   // (last: it marks the set as complete)
}

void drop_graphs(dhw_handle* h) {
  for (auto& kv : h->graphs) hipGraphExecDestroy(kv.second);
  h->graphs.clear();
  h->graph_plane_gen.clear();
  plane_invalidate(h);   // (every caller is an event after which the resident plane may be stale: new weights, a persistent-step fallback)
}

static int act_alloc(dhw_handle* h, void** slot, long rows, int cols, bool f32 = false) {
  const size_t bytes = (size_t)(rows + SLACK_ROWS) * cols * (f32 ? 4 : h->es);
  return dev_alloc(h, slot, bytes, true);
}

static int pad32(int x) { return ((x + 31) / 32) * 32; }

// width of EncoderLayer li (0 = enc3 at c2, 1 = enc5 at c3, the bottleneck layers at 2 c2) and its stroke rows at length L
static int el_width(const dhw_dims& d, int li) { return li == 0 ? d.c2 : li == 1 ? d.c3 : 2 * d.c2; }
long el_rows(long L, int li) { return li == 0 ? L / 2 : li == 1 ? L / 4 : L / 8; }

int alloc_workspace(dhw_handle* h, Workspace& w, long B) {
  w.cap_B = B;
  const dhw_dims& d = h->dims;
  const long L = d.max_L, Lt = d.max_Lt, S5 = d.S * 5;
  const int c1 = d.c1, c2 = d.c2, c3 = d.c3, dt = 2 * c2;
  int rc;
#define AA(slot, rows, cols) if ((rc = act_alloc(h, &(slot), rows, cols))) return rc
  AA(w.sty_in, B * S5, STYLE_CH); AA(w.sty_h, B * S5, 4 * c2); AA(w.sty_n, B * S5, dt); AA(w.ts.s1, B * S5, dt);
  AA(w.ts.k8, B * S5, dt);
  AA(w.t_n, B * Lt, dt); AA(w.ts.t1, B * Lt, dt); AA(w.ts.q8, B * Lt, dt); AA(w.ts.a8, B * Lt, dt); AA(w.ts.t2, B * Lt, dt);
  AA(w.ts.tf_h, B * Lt, 2 * dt); AA(w.ts.text_out, B * Lt, dt);
  h->lpadS = pad32((int)S5);
  h->lpadT = pad32((int)Lt);
  AA(w.ts.vt8, B * dt, h->lpadS);
  AA(w.x0, B * L, c1);
  struct CB { long rows; int cout; };
  const CB cbs[CB_N] = {{L, c1}, {L / 2, c2}, {L / 4, c3}, {L / 4, c3}, {L / 2, c2}, {L, c1}};
  for (int i = 0; i < CB_N; ++i) {
    const CB& c = cbs[i];
    AA(w.cb[i].h1, B * c.rows, c.cout / 2);
    AA(w.cb[i].h2, B * c.rows, c.cout);
    if (i == CB_DEC1) { if ((rc = act_alloc(h, &w.cb[i].out, B * c.rows, c.cout, true))) return rc; }   // dec1's output feeds the heads in fp32
    else AA(w.cb[i].out, B * c.rows, c.cout);
  }
  AA(w.enc1_pool, B * L / 2, c1);
  h->lpadX[0] = pad32((int)(L / 2));
  h->lpadX[1] = pad32((int)(L / 4));
  h->lpadX[2] = pad32((int)(L / 8));
  w.el.assign(2 + d.num_layers, EncBufs{});
  for (size_t i = 0; i < w.el.size(); ++i) {
    EncBufs& e = w.el[i];
    const int dm = el_width(d, (int)i), lp = h->lpadX[i < 2 ? i : 2];
    const long rows = el_rows(L, (int)i);
    AA(e.t.tl, B * Lt, dm); AA(e.t.k1, B * Lt, dm); AA(e.t.vt1, B * dm, h->lpadT);
    AA(e.q1, B * rows, dm); AA(e.a1, B * rows, dm); AA(e.x2, B * rows, dm);
    // (qk2: the bf16 fused kernels keep [q2 | k2 | v2] rows; the other paths use 2 dm columns of it and the transposed vt2)
    AA(e.qk2, B * rows, 3 * dm); AA(e.vt2, B * dm, lp); AA(e.a2, B * rows, dm);
    AA(e.x3, B * rows, dm); AA(e.f, B * rows, 2 * dm); AA(e.out, B * rows, dm);
  }
  AA(w.enc3_pool, B * L / 4, c2); AA(w.enc5_pool, B * L / 8, c3);
  AA(w.att_dense, B * L / 8, dt);
  AA(w.xd[0], B * L / 4, dt); AA(w.xd[1], B * L / 2, c3); AA(w.xd[2], B * L, c2);
#undef AA
  if ((rc = dev_alloc(h, (void**)&w.d_xt, (size_t)(B * L + SLACK_ROWS) * 2 * 4))) return rc;
  return 0;
}

// All-steps text plane: every sigma-dependent text-side activation for `steps` sampler steps x `B` prompts.
int ensure_plane(dhw_handle* h, Workspace& w, long steps, long B) {
  if (steps * B <= w.plane_cap) return 0;
  const dhw_dims& d = h->dims;
  const long n = steps * B, Lt = d.max_Lt, S5 = d.S * 5;
  const int dt = 2 * d.c2;
  int rc;
#define AA(slot, rows, cols) if ((rc = act_alloc(h, &(slot), rows, cols))) return rc
  // with the fused text-side kernels (every call of this handle qualifies) only text_out and the layers' K / V exist
  const bool fused = h->fuse && h->fuse_text && textside_supported(h->prec, (int)Lt, (int)S5, dt);
  if (!fused) {
    AA(w.tsT.s1, n * S5, dt); AA(w.tsT.k8, n * S5, dt); AA(w.tsT.vt8, n * dt, h->lpadS);
    AA(w.tsT.t1, n * Lt, dt); AA(w.tsT.q8, n * Lt, dt); AA(w.tsT.a8, n * Lt, dt); AA(w.tsT.t2, n * Lt, dt);
    AA(w.tsT.tf_h, n * Lt, 2 * dt);
  }
  AA(w.tsT.text_out, n * Lt, dt);
  for (size_t i = 0; i < w.el.size(); ++i) {
    const int dm = el_width(d, (int)i);
    if (!fused) AA(w.el[i].tT.tl, n * Lt, dm);
    AA(w.el[i].tT.k1, n * Lt, dm); AA(w.el[i].tT.vt1, n * dm, h->lpadT);
  }
#undef AA
  w.plane_cap = n;   // (a grown plane leaks the smaller one until destroy)
  ++h->plane_gen;    // new, zeroed ".T" buffers: nothing resident (graphs captured earlier keep writing and reading the old ones)
  plane_invalidate(h);
  return 0;
}

int alloc_shared(dhw_handle* h) {
  const dhw_dims& d = h->dims;
  const long B = d.max_B, L = d.max_L, Lt = d.max_Lt, S5 = d.S * 5;
  int rc;
  if ((rc = dev_alloc(h, (void**)&h->d_sigma_in, B * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_sig32, B * SIG * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_film, (size_t)B * 2 * h->film_tot * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_seed, 16))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_plane_skip, 8))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_text_stage, (size_t)(B * Lt + 64) * 8))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_style_stage, (size_t)(B * S5 + SLACK_ROWS) * STYLE_CH * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_out_stage, (size_t)(B * L + SLACK_ROWS) * 3 * 4))) return rc;
  if ((rc = dev_alloc(h, (void**)&h->d_lens, (size_t)B * 4))) return rc;
  if (hipHostMalloc((void**)&h->h_lens_pin, (size_t)B * 4) != hipSuccess) return fail(h, DHW_ERR_HIP, "pinned length buffer: %s", hipGetErrorString(hipGetLastError()));
  if (hipEventCreateWithFlags(&h->lens_ev, hipEventDisableTiming) != hipSuccess) return fail(h, DHW_ERR_HIP, "event create failed");
  return 0;
}

// Names are resolved HERE, once per handle: the EncoderLayers' module names and the table dhw_debug_read searches.
void build_names(dhw_handle* h) {
  const int nel = 2 + h->dims.num_layers;
  h->el_name.clear();
  h->el_name.push_back("enc3");
  h->el_name.push_back("enc5");
  for (int i = 0; i < h->dims.num_layers; ++i) h->el_name.push_back("att_layers." + std::to_string(i));
  h->taps.assign(TAP_CONV0 + CB_N + TAPS_PER_EL * nel, TapSlot{});
  h->taps[TAP_SIGMA_FFN].name = "sigma_ffn";
  h->taps[TAP_INPUT_DENSE].name = "input_dense";
  h->taps[TAP_TS].name = "text_style_model";
  h->taps[TAP_TS_STYLE].name = "text_style_model.style";
  h->taps[TAP_TS_T2].name = "text_style_model.t2";
  h->taps[TAP_ATT_DENSE].name = "att_dense";
  h->taps[TAP_UP3].name = "skip_conv3+up";
  h->taps[TAP_UP2].name = "skip_conv2+up";
  h->taps[TAP_UP1].name = "skip_conv1+up";
  h->taps[TAP_POOL1].name = "enc1.pool";
  h->taps[TAP_POOL3].name = "enc3.pool";
  h->taps[TAP_POOL5].name = "enc5.pool";
  for (int i = 0; i < CB_N; ++i) h->taps[tap_conv(i)].name = kConvName[i];
  for (int li = 0; li < nel; ++li) {
    h->taps[tap_el(li, 0)].name = h->el_name[li];
    h->taps[tap_el(li, 1)].name = h->el_name[li] + ".x2";
    h->taps[tap_el(li, 2)].name = h->el_name[li] + ".x3";
    h->taps[tap_el(li, 3)].name = h->el_name[li] + ".k1";   // the layer's text keys [Lt, d]
    h->taps[tap_el(li, 4)].name = h->el_name[li] + ".v1";   // its text values as stored: rows [Lt, d] (v_rows) or V^T [d, lpadT]
  }
}

// Every per-call buffer of a freshly allocated workspace must exist (the all-steps plane comes later, ensure_plane): a buffer
// the allocation code forgot is a dhw_create error, not something a launch discovers.
int verify_workspace(dhw_handle* h, const Workspace& w) {
  std::vector<std::pair<const char*, const void*>> all = {
      {"sty_in", w.sty_in}, {"sty_h", w.sty_h}, {"sty_n", w.sty_n}, {"t_n", w.t_n}, {"s1", w.ts.s1}, {"k8", w.ts.k8}, {"vt8", w.ts.vt8},
      {"t1", w.ts.t1}, {"q8", w.ts.q8}, {"a8", w.ts.a8}, {"t2", w.ts.t2}, {"tf_h", w.ts.tf_h}, {"text_out", w.ts.text_out}, {"x0", w.x0},
      {"enc1.pool", w.enc1_pool}, {"enc3.pool", w.enc3_pool}, {"enc5.pool", w.enc5_pool}, {"att_dense", w.att_dense},
      {"xd3", w.xd[0]}, {"xd2", w.xd[1]}, {"xd1", w.xd[2]}, {"x_t", w.d_xt}};
  for (int i = 0; i < CB_N; ++i) { all.push_back({"convblock h1", w.cb[i].h1}); all.push_back({"convblock h2", w.cb[i].h2}); all.push_back({"convblock out", w.cb[i].out}); }
  if ((int)w.el.size() != 2 + h->dims.num_layers) return fail(h, DHW_ERR_INTERNAL, "internal: workspace has %d EncoderLayers, the model %d", (int)w.el.size(), 2 + h->dims.num_layers);
  for (const EncBufs& e : w.el)
    for (auto kv : std::initializer_list<std::pair<const char*, const void*>>{{"tl", e.t.tl}, {"k1", e.t.k1}, {"vt1", e.t.vt1}, {"q1", e.q1}, {"a1", e.a1}, {"x2", e.x2},
                                                                               {"qk2", e.qk2}, {"vt2", e.vt2}, {"a2", e.a2}, {"x3", e.x3}, {"f", e.f}, {"out", e.out}})
      all.push_back(kv);
  for (auto& kv : all)
    if (!kv.second) return fail(h, DHW_ERR_INTERNAL, "internal: workspace buffer '%s' was not allocated", kv.first);
  return 0;
}

void destroy_impl(dhw_handle* h) {
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  drop_graphs(h);
  for (auto& r : h->prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (int i = 1; i < MAX_STREAMS; ++i)
    if (h->sub_streams[i]) hipStreamDestroy(h->sub_streams[i]);
  h->arena.free_all();
  if (h->h_step_err) hipHostFree(h->h_step_err);
  if (h->h_lens_pin) hipHostFree(h->h_lens_pin);
  if (h->h_prof_skip) hipHostFree(h->h_prof_skip);
  if (h->lens_ev) hipEventDestroy(h->lens_ev);
  if (h->h_guide_scale_pin) hipHostFree(h->h_guide_scale_pin);
  if (h->guide_ev) hipEventDestroy(h->guide_ev);
  delete h;
}
