// Where everything lives: the parameter layout of the flat buffers (build_layout) and the workspace plans of the fp32 and the bf16
// model (build_plan, build_plan16) with the decode areas they share.
#include "skf_model_internal.h"

namespace skf_model_detail {
namespace {

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

void add_entry(Layout& L, const std::string& name, size_t off, int rows, int cols, int stride) {
  SkfParamEntry e;
  memset(&e, 0, sizeof(e));
  snprintf(e.name, sizeof(e.name), "%s", name.c_str());
  e.offset = (int64_t)off; e.rows = rows; e.cols = cols; e.row_stride = stride;
  L.entries.push_back(e);
}

size_t alloc(Layout& L, size_t n) { size_t o = L.total; L.total += pad4(n); return o; }

DenseP dense(Layout& L, const std::string& name, int in, int out) {
  DenseP d; d.in = in; d.out = out; d.ld = out;
  d.w = alloc(L, (size_t)in * out); d.b = alloc(L, out);
  add_entry(L, name + "/kernel", d.w, in, out, out);
  add_entry(L, name + "/bias", d.b, 1, out, out);
  return d;
}

// fused [in][nparts*out] block exposed as nparts strided (in,out) kernels
DenseP fused_dense(Layout& L, const std::string& prefix, const char* const* names, int nparts, int in, int out) {
  DenseP d; d.in = in; d.out = nparts * out; d.ld = nparts * out;
  d.w = alloc(L, (size_t)in * d.out); d.b = alloc(L, d.out);
  for (int i = 0; i < nparts; ++i) {
    add_entry(L, prefix + "/" + names[i] + "/kernel", d.w + (size_t)i * out, in, out, d.ld);
    add_entry(L, prefix + "/" + names[i] + "/bias", d.b + (size_t)i * out, 1, out, out);
  }
  return d;
}

LnP lnp(Layout& L, const std::string& name, int d) {
  LnP p; p.g = alloc(L, d); p.b = alloc(L, d);
  add_entry(L, name + "/gamma", p.g, 1, d, d);
  add_entry(L, name + "/beta", p.b, 1, d, d);
  return p;
}

}  // namespace

Layout build_layout(const SkfConfig& c) {
  Layout L;
  const int d = c.d_model;
  // SelfAttnV1 returns (B,d), V2 projects to (B,lowerdim); without a bottleneck the "embedding" is the encoder output
  const int E = (has_bott(c) && c.attn_version == 2) ? c.lowerdim : d;
  const int Ua = c.attn_version == 2 ? d : c.lowerdim;    // W_attn is (d,units) in V1, (d,d) in V2
  L.E = E; L.Ua = Ua;
  static const char* const qkv_names[3] = {"wq", "wk", "wv"};
  static const char* const kv_names[2] = {"wk", "wv"};
  if (c.continuous) {
    L.enc_embd = dense(L, "encoder/embedding", 5, d);
  } else {
    L.enc_emb = alloc(L, (size_t)c.vocab_size * d);
    add_entry(L, "encoder/embedding", L.enc_emb, c.vocab_size, d, d);
  }
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string p = "encoder/layer" + std::to_string(i);
    EncLayerP e;
    e.mha.qkv = fused_dense(L, p + "/mha", qkv_names, 3, d, d);
    e.mha.o = dense(L, p + "/mha/dense", d, d);
    e.f1 = dense(L, p + "/ffn/dense1", d, c.dff);
    e.f2 = dense(L, p + "/ffn/dense2", c.dff, d);
    e.ln1 = lnp(L, p + "/layernorm1", d);
    e.ln2 = lnp(L, p + "/layernorm2", d);
    L.enc.push_back(e);
  }
  if (has_bott(c)) {
    L.bott_w.in = d; L.bott_w.out = Ua; L.bott_w.ld = Ua;
    L.bott_w.w = alloc(L, (size_t)d * Ua); L.bott_w.b = alloc(L, Ua);
    L.bott_v = alloc(L, Ua);
    add_entry(L, "bottleneck/W_attn", L.bott_w.w, d, Ua, Ua);
    add_entry(L, "bottleneck/b_attn", L.bott_w.b, 1, Ua, Ua);
    add_entry(L, "bottleneck/V_attn", L.bott_v, Ua, 1, 1);
    if (c.attn_version == 2) L.bott_e = dense(L, "bottleneck/embeding_layer", d, c.lowerdim);
  }
  if (has_cls(c)) {
    for (int i = 0; i < c.class_buffer_layers; ++i)
      L.cbuf.push_back(dense(L, "class_buffer/" + std::to_string(i), i == 0 ? E : c.lowerdim, c.lowerdim));
    L.cls = dense(L, "classify", c.class_buffer_layers ? c.lowerdim : E, c.n_classes);
  }
  L.dec_off = L.total;                   // first float of the decoder-side variables (gradient bucket boundary)
  if (!do_recon(c)) return L;
  if (has_bott(c)) {
    L.exp_w = alloc(L, c.seq_len); L.exp_b = alloc(L, c.seq_len);
    add_entry(L, "expand/kernel", L.exp_w, 1, c.seq_len, c.seq_len);
    add_entry(L, "expand/bias", L.exp_b, 1, c.seq_len, c.seq_len);
  }
  L.dec_off = L.total;
  if (c.continuous) {
    L.dec_embd = dense(L, "decoder/embedding", 5, d);
  } else {
    L.dec_emb = alloc(L, (size_t)c.vocab_size * d);
    add_entry(L, "decoder/embedding", L.dec_emb, c.vocab_size, d, d);
  }
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string p = "decoder/layer" + std::to_string(i);
    DecLayerP e;
    e.mha1.qkv = fused_dense(L, p + "/mha1", qkv_names, 3, d, d);
    e.mha1.o = dense(L, p + "/mha1/dense", d, d);
    e.mha2.q = dense(L, p + "/mha2/wq", d, d);
    e.mha2.kv = fused_dense(L, p + "/mha2", kv_names, 2, E, d);
    e.mha2.o = dense(L, p + "/mha2/dense", d, d);
    e.f1 = dense(L, p + "/ffn/dense1", d, c.dff);
    e.f2 = dense(L, p + "/ffn/dense2", c.dff, d);
    e.ln1 = lnp(L, p + "/layernorm1", d);
    e.ln2 = lnp(L, p + "/layernorm2", d);
    e.ln3 = lnp(L, p + "/layernorm3", d);
    L.dec.push_back(e);
  }
  L.out = dense(L, "output", d, c.continuous ? 5 : c.vocab_size);
  return L;
}

namespace {
DecodeAreas take_decode_areas(Bump& b, const SkfConfig& c, bool own_cross) {
  DecodeAreas A;
  const size_t B = c.batch, L = c.seq_len, d = c.d_model, f = sizeof(float);
  if (own_cross) A.pre = b.take(B * L * d * f);
  for (int i = 0; i < c.num_layers; ++i) {
    if (own_cross) A.kv2.push_back(b.take(B * L * 2 * d * f));
    A.cache.push_back(b.take(B * L * 2 * d * f));
  }
  A.img = b.take(B * (L + 1) * (c.continuous ? 5 * f : 8));
  A.mask = b.take(B * (L + 1)); A.flags = b.take((B + 16) * sizeof(int));
  A.limit = b.take(2 * B * sizeof(int));
  A.dyn = b.take(64);
  A.anc = b.take(2 * B * (L + 1) * sizeof(int));
  A.cand = b.take(2 * B * SKF_BEAM_MAX * sizeof(float));
  A.beam = b.take(3 * B * sizeof(int));
  if (!c.continuous) {
    A.pfx_tok = b.take(B * L * 8); A.pfx_len = b.take(2 * B * sizeof(int));
  }
  return A;
}

}  // namespace

// Every area allocated (offset 0 is the staged input, so an area left at its default would alias it), in allocation order, none
// overlapping the next, inside the plan.  Checked once when a model is created.
bool decode_areas_ok(const DecodeAreas& A, size_t plan_bytes) {
  std::vector<size_t> o;
  if (!A.kv2.empty()) o.push_back(A.pre);
  for (size_t i = 0; i < A.cache.size(); ++i) {
    if (!A.kv2.empty()) o.push_back(A.kv2[i]);
    o.push_back(A.cache[i]);
  }
  for (size_t v : {A.img, A.mask, A.flags, A.limit, A.dyn, A.anc, A.cand, A.beam}) o.push_back(v);
  if (A.pfx_tok) for (size_t v : {A.pfx_tok, A.pfx_len}) o.push_back(v);      // (token models)
  if (o[0] == 0 || o.back() + 64 > plan_bytes || (!A.kv2.empty() && A.kv2.size() != A.cache.size())) return false;
  for (size_t i = 1; i < o.size(); ++i)
    if (o[i] <= o[i - 1]) return false;
  return true;
}

namespace {
size_t wgrad_ws(int in, int out, int rows) {
  return skf_gemm_workspace_bytes(in, out, rows, skf_gemm_default_splits(in, out, rows), 1);
}

}  // namespace
Plan build_plan(const SkfConfig& c) {
  Plan P;
  Bump b;
  const size_t B = c.batch, L = c.seq_len, Ld = c.seq_len - 1, d = c.d_model, F = c.dff, U = c.lowerdim;
  const size_t Me = B * L, Md = B * Ld, H = c.num_heads, f = sizeof(float);
  const size_t E = (has_bott(c) && c.attn_version == 2) ? U : d, Ua = c.attn_version == 2 ? d : U;
  const size_t in_bytes = c.continuous ? B * L * 5 * 4 : B * L * 8;   // (B,L,5) f32 or (B,L) i64
  const size_t Vout = c.continuous ? 5 : (size_t)c.vocab_size;
  P.inp = b.take(in_bytes); P.tar = b.take(in_bytes); P.labels = b.take(B * 8);
  P.enc_mask = b.take(B * L); P.dec_mask = b.take(B * L);
  for (int i = 0; i < c.num_layers; ++i) {
    EncAct a;
    a.x_in = b.take(Me * d * f); a.qkv = b.take(Me * 3 * d * f); a.o = b.take(Me * d * f); a.z1 = b.take(Me * d * f);
    a.st1 = b.take(Me * 2 * f); a.astats = b.take(B * H * L * 2 * f); a.x1 = b.take(Me * d * f);
    a.h = b.take(Me * F * f); a.z2 = b.take(Me * d * f); a.st2 = b.take(Me * 2 * f);
    a.hbits = b.take(std::max(skf_gemm_relu_bits_bytes((int)Me, (int)F, (int)d, c.gemm_precision),        // 0 bytes: no sign-bit path for this shape
                              skf_ffn_relu_bits_bytes((int)Me, (int)d, (int)F, c.gemm_precision)));
    a.img[0] = b.take(skf_ffn_image_bytes((int)d, (int)F, c.gemm_precision)); a.img[1] = b.take(skf_ffn_image_bytes((int)d, (int)F, c.gemm_precision));
    a.img_o = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision));
    a.img_qkv = b.take(skf_dense_image_bytes((int)d, 3 * (int)d, c.gemm_precision));
    a.img_of = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision));
    a.x2 = 0;
    P.enc.push_back(a);
  }
  const size_t enc_out = b.take(Me * d * f);
  for (int i = 0; i < c.num_layers; ++i) P.enc[i].x2 = (i + 1 < c.num_layers) ? P.enc[i + 1].x_in : enc_out;
  P.u = b.take(Me * Ua * f); P.pool_a = b.take(B * L * f); P.emb = b.take(B * E * f);
  P.pooled = b.take(B * d * f); P.dpooled = b.take(B * d * f);
  for (int i = 0; i < c.class_buffer_layers; ++i) { P.cb_h.push_back(b.take(B * U * f)); P.cb_f.push_back(b.take(B * U * f)); }
  P.dcb[0] = b.take(B * U * f); P.dcb[1] = b.take(B * U * f);
  P.cls_logits = b.take(B * c.n_classes * f); P.cls_probs = b.take(B * c.n_classes * f);
  P.pre = b.take(Me * E * f);
  for (int i = 0; i < c.num_layers; ++i) {
    DecAct a;
    a.x_in = b.take(Md * d * f); a.qkv = b.take(Md * 3 * d * f); a.o1 = b.take(Md * d * f); a.z1 = b.take(Md * d * f);
    a.st1 = b.take(Md * 2 * f); a.astats1 = b.take(B * H * Ld * 2 * f); a.out1 = b.take(Md * d * f);
    a.q2 = b.take(Md * d * f); a.kv2 = b.take(Me * 2 * d * f); a.o2 = b.take(Md * d * f);   // kv2 = pre (Me,E) . Wkv (E,2d)
    a.astats2 = b.take(B * H * Ld * 2 * f); a.z2 = b.take(Md * d * f); a.st2 = b.take(Md * 2 * f);
    a.out2 = b.take(Md * d * f); a.h = b.take(Md * F * f); a.z3 = b.take(Md * d * f); a.st3 = b.take(Md * 2 * f);
    a.hbits = b.take(std::max(skf_gemm_relu_bits_bytes((int)Md, (int)F, (int)d, c.gemm_precision),
                              skf_ffn_relu_bits_bytes((int)Md, (int)d, (int)F, c.gemm_precision)));
    a.img[0] = b.take(skf_ffn_image_bytes((int)d, (int)F, c.gemm_precision)); a.img[1] = b.take(skf_ffn_image_bytes((int)d, (int)F, c.gemm_precision));
    a.img_o1 = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision)); a.img_o2 = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision));
    a.img_qkv = b.take(skf_dense_image_bytes((int)d, 3 * (int)d, c.gemm_precision));
    a.img_o2f = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision));
    a.img_o1f = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision)); a.img_q2 = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision));
    a.img_q2t = b.take(skf_dense_image_bytes((int)d, (int)d, c.gemm_precision));
    a.out3 = 0;
    P.dec.push_back(a);
  }
  const size_t dec_out = b.take(Md * d * f);
  for (int i = 0; i < c.num_layers; ++i) P.dec[i].out3 = (i + 1 < c.num_layers) ? P.dec[i + 1].x_in : dec_out;
  P.logits = b.take(Md * Vout * f);
  P.recon_loss = b.take(Md * f); P.recon_hit = b.take(Md * f); P.cls_loss = b.take(B * f); P.cls_hit = b.take(B * f);
  P.row_mask = b.take(Md * f); P.cont_scal = b.take(64);
  P.gA = b.take(Me * d * f); P.gB = b.take(Me * d * f); P.gC = b.take(Me * d * f);
  P.dqkv = b.take(Me * 3 * d * f); P.dh = b.take(Me * F * f); P.do_ = b.take(Me * d * f);
  P.dpre = b.take(Me * E * f); P.dkv2 = b.take(Me * 2 * d * f); P.dq2 = b.take(Md * d * f); P.demb = b.take(B * E * f);
  // A layer's weight gradients (side stream) read its dy / dh / dq|k|v buffers long after the main stream has moved on, so the buffers
  // rotate.  With two sets the main stream waits for the group of two layers ago in front of every layer - finished long since, but a
  // wait in the queue costs the waiting stream ~6 us whether or not it has to wait (tools/wait_cost.py).  One set per layer: no buffer
  // is written twice in a step and those waits are gone (cfg 2: 8 x 170 MB); above 8 GB the sets fall back to two.
  {
    const size_t per_set = (3 * Me * d + Me * F + Md * d + Me * 2 * d + Me * 3 * d) * f;
    const size_t layers = (size_t)c.num_layers * (do_recon(c) ? 2 : 1);
    P.n_gs = (per_set * layers > ((size_t)8 << 30) || layers < 2) ? 2 : (int)layers;
    P.gs.resize(P.n_gs);
  }
  for (int k = 0; k < P.n_gs; ++k) {
    for (int j = 0; j < 3; ++j) P.gs[k].dy[j] = b.take(Me * d * f);
    P.gs[k].dh = k == 0 ? P.dh : b.take(Me * F * f);
    P.gs[k].dq2 = k == 0 ? P.dq2 : b.take(Md * d * f);
    P.gs[k].dkv2 = k == 0 ? P.dkv2 : b.take(Me * 2 * d * f);
    P.gs[k].dqkv = k == 0 ? P.dqkv : b.take(Me * 3 * d * f);
  }
  size_t g = 0;
  auto mx = [&](size_t v) { if (v > g) g = v; };
  mx(wgrad_ws(d, 3 * d, Me)); mx(wgrad_ws(d, d, Me)); mx(wgrad_ws(d, F, Me)); mx(wgrad_ws(F, d, Me));
  mx(wgrad_ws((int)E, 2 * d, Me)); mx(wgrad_ws(d, (int)Vout, Md));
  if (has_bott(c)) {
    mx(wgrad_ws(d, (int)Ua, Me));
    mx(wgrad_ws((int)E, c.n_classes, B)); mx(wgrad_ws(U, c.n_classes, B)); mx(wgrad_ws(d, U, B)); mx(wgrad_ws((int)E, U, B)); mx(wgrad_ws(U, U, B));
  }
  P.gemm_ws_bytes = g; P.gemm_ws = b.take(g);
  P.n_wgrads = 4 + 11 * (size_t)c.num_layers + (size_t)c.class_buffer_layers + 5 * (size_t)c.num_layers + 3;   // + one entry per LayerNorm + expander (2) / pooling (1) partials
  // per-sample partials of the expander's kernel / bias gradients [2][B][L] and of the pooling scorer's V gradient [B][Ua]: column
  // sums in the batched reduction instead of three one-workgroup launches on the main stream between the decoder and encoder backward
  P.bott_part = b.take((2 * B * L + B * 4096) * f);
  P.ln_part_stride = (skf_layernorm_bwd_workspace_bytes((int)Me, (int)d) + 255) & ~(size_t)255;
  P.ln_part = b.take(5 * (size_t)c.num_layers * P.ln_part_stride);
  P.slab_arena_bytes = P.n_wgrads * ((g + 255) & ~(size_t)255);
  P.slab_arena = b.take(P.slab_arena_bytes);
  P.descs = b.take(P.n_wgrads * sizeof(SkfReduceDesc));
  size_t s = skf_layernorm_bwd_workspace_bytes((int)Me, (int)d);
  if (B * Ua * f > s) s = B * Ua * f;
  if (2 * B * L * f > s) s = 2 * B * L * f;
  if (c.continuous && skf_embed_continuous_bwd_workspace_bytes((int)Me, (int)d) > s) s = skf_embed_continuous_bwd_workspace_bytes((int)Me, (int)d);
  P.small_ws_bytes = s; P.small_ws = b.take(s);
  if (!c.continuous && c.vocab_size <= 12288 && c.d_model <= 512) {   // (the sorted kernel's partial slab is sized for rows of <= 512 floats)
    P.emb_sort_bytes = (skf_embed_sort_workspace_bytes((int)B, (int)L, c.vocab_size) + 255) & ~(size_t)255;
    P.emb_sort[0] = b.take(P.emb_sort_bytes); P.emb_sort[1] = b.take(P.emb_sort_bytes);
  }
  P.dca = take_decode_areas(b, c, false);          // (pre_decoder and the cross K|V are the training buffers P.pre / P.dec[l].kv2)
  P.dc_x[0] = b.take(B * d * f); P.dc_x[1] = b.take(B * d * f); P.dc_q = b.take(B * d * f); P.dc_o = b.take(B * d * f);
  P.dc_z = b.take(B * d * f); P.dc_out1 = b.take(B * d * f); P.dc_out2 = b.take(B * d * f); P.dc_h = b.take(B * F * f);
  P.dc_logits = b.take(B * Vout * f); P.dc_stats = b.take(B * 2 * f); P.dc_kvnew = b.take(B * 2 * d * f);
  P.live_len = b.take(B * sizeof(int));
  P.order = b.take(B * sizeof(int));
  P.live16 = b.take(skf_row_blocks_bytes(B * (L - 1), 16)); P.live32 = b.take(skf_row_blocks_bytes(B * (L - 1), 32));
  P.bytes = b.off;
  return P;
}

// ------------------------------------------------------------------ bf16 workspace plan
namespace {

inline int pad8(int n) { return (n + 7) & ~7; }

void add_img(Plan16& P, Bump& b, const DenseP& w) {
  Img16 im;
  im.in = w.in; im.out = w.out; im.ld_src = w.ld; im.src = w.w;
  im.ldw = pad8(w.out); im.ldt = pad8(w.in);
  im.w = b.take((size_t)w.in * im.ldw * 2);
  im.wt = b.take((size_t)w.out * im.ldt * 2);
  P.img[w.w] = im;
}

}  // namespace

Plan16 build_plan16(const SkfConfig& c, const Layout& L) {
  Plan16 P;
  Bump b;
  const size_t B = c.batch, Ls = c.seq_len, Ld = c.seq_len - 1, d = c.d_model, F = c.dff, U = c.lowerdim;
  const size_t Me = B * Ls, Md = B * Ld, H = c.num_heads, f = sizeof(float), h2 = 2;
  const int N = c.num_layers;
  P.inp = b.take(B * Ls * 8); P.tar = b.take(B * Ls * 8); P.labels = b.take(B * 8);
  P.enc_mask = b.take(B * Ls); P.dec_mask = b.take(B * Ls);
  for (int i = 0; i < N; ++i) {
    Enc16 a;
    a.x_in = b.take(Me * d * h2); a.qkv = b.take(Me * 3 * d * h2); a.o = b.take(Me * d * h2); a.olo = b.take(Me * d * h2); a.z1 = b.take(Me * d * h2);
    a.st1 = b.take(Me * 2 * f); a.astats = b.take(B * H * Ls * 2 * f); a.x1 = b.take(Me * d * h2);
    a.h = b.take(Me * F * h2); a.z2 = b.take(Me * d * h2); a.st2 = b.take(Me * 2 * f); a.x2 = 0;
    a.hbits = b.take(skf_gemm_bf16_relu_bits_bytes((int)Me, (int)F));      // sign bits of h for the ffn input gradient (0 bytes: dff % 8 != 0)
    P.enc.push_back(a);
  }
  const size_t enc_out = b.take(Me * d * h2);
  for (int i = 0; i < N; ++i) P.enc[i].x2 = (i + 1 < N) ? P.enc[i + 1].x_in : enc_out;
  P.u = b.take(Me * U * h2); P.pool_a = b.take(B * Ls * f); P.emb = b.take(B * d * f);
  P.cls_logits = b.take(B * c.n_classes * f); P.cls_probs = b.take(B * c.n_classes * f);
  P.pre = b.take(Me * d * h2);
  for (int i = 0; i < N; ++i) {
    Dec16 a;
    a.x_in = b.take(Md * d * h2); a.qkv = b.take(Md * 3 * d * h2); a.o1 = b.take(Md * d * h2); a.olo1 = b.take(Md * d * h2); a.z1 = b.take(Md * d * h2);
    a.st1 = b.take(Md * 2 * f); a.astats1 = b.take(B * H * Ld * 2 * f); a.out1 = b.take(Md * d * h2);
    a.q2 = b.take(Md * d * h2); a.kv2 = b.take(Me * 2 * d * h2); a.o2 = b.take(Md * d * h2); a.olo2 = b.take(Md * d * h2);
    a.astats2 = b.take(B * H * Ld * 2 * f); a.z2 = b.take(Md * d * h2); a.st2 = b.take(Md * 2 * f);
    a.out2 = b.take(Md * d * h2); a.h = b.take(Md * F * h2); a.z3 = b.take(Md * d * h2); a.st3 = b.take(Md * 2 * f);
    a.hbits = b.take(skf_gemm_bf16_relu_bits_bytes((int)Md, (int)F));
    a.out3 = 0;
    P.dec.push_back(a);
  }
  const size_t dec_out = b.take(Md * d * h2);
  for (int i = 0; i < N; ++i) P.dec[i].out3 = (i + 1 < N) ? P.dec[i + 1].x_in : dec_out;
  P.ld_logits = pad8(c.vocab_size);
  P.logits = b.take(Md * (size_t)P.ld_logits * h2);
  P.recon_loss = b.take(Md * f); P.recon_hit = b.take(Md * f); P.cls_loss = b.take(B * f); P.cls_hit = b.take(B * f);
  P.gA = b.take(Me * d * h2); P.gB = b.take(Me * d * h2); P.dy = b.take(Me * d * h2); P.dO = b.take(Me * d * h2);
  P.dqkv = b.take(Me * 3 * d * h2); P.dh = b.take(Me * F * h2); P.dpre = b.take(Me * d * h2);
  P.dkv2 = b.take(Me * 2 * d * h2); P.dq2 = b.take(Md * d * h2); P.demb = b.take(B * d * f);
  // weight-gradient slab: the largest (in, out) pair of the model at its default split count
  size_t g = 0;
  auto mx = [&](int in, int out, size_t rows) {
    const size_t v = skf_gemm_bf16_wgrad_workspace_bytes(in, out, (int)rows, skf_gemm_bf16_wgrad_splits(in, out, (int)rows));
    if (v > g) g = v;
  };
  mx((int)d, (int)(3 * d), Me); mx((int)d, (int)d, Me); mx((int)d, (int)F, Me); mx((int)F, (int)d, Me); mx((int)d, (int)(2 * d), Me);
  mx((int)d, c.vocab_size, Md); mx((int)d, (int)U, Me);
  const size_t small = skf_gemm_workspace_bytes((int)d, c.n_classes, (int)B, 8, 1);
  if (small > g) g = small;
  P.slab_bytes = g; P.slab = b.take(g);
  size_t s = B * U * f;
  if (2 * B * Ls * f > s) s = 2 * B * Ls * f;
  P.small_ws_bytes = s; P.small_ws = b.take(s);
  P.attn_ws_bytes = skf_attention_bf16_bwd_workspace_bytes((int)B, (int)H, (int)Ls); P.attn_ws = b.take(P.attn_ws_bytes);
  P.ln_ws_bytes = skf_layernorm_bwd_bf16_workspace_bytes((int)Me, (int)d); P.ln_ws = b.take(P.ln_ws_bytes);
  P.cast_descs_bytes = 256 * sizeof(SkfCastDesc); P.cast_descs = b.take(P.cast_descs_bytes);
  P.ln_n = 5 * (int)c.num_layers; P.ln_n_dec = 3 * (int)c.num_layers;
  P.ln_slabs = b.take((size_t)P.ln_n * P.ln_ws_bytes); P.ln_descs = b.take((size_t)P.ln_n * sizeof(SkfReduceDesc));
  P.dca = take_decode_areas(b, c, true);
  P.live_len = b.take(B * sizeof(int));
  P.order = b.take(B * sizeof(int));
  P.live1 = b.take(skf_row_blocks_bytes((int)Md, 1)); P.live64 = b.take(skf_row_blocks_bytes((int)Md, 64));
  if (c.vocab_size <= 12288) {
    P.emb_sort_bytes = (skf_embed_sort_workspace_bytes((int)B, (int)Ls, c.vocab_size) + 255) & ~(size_t)255;
    P.emb_sort[0] = b.take(P.emb_sort_bytes); P.emb_sort[1] = b.take(P.emb_sort_bytes);
  }
  for (const auto& e : L.enc) { add_img(P, b, e.mha.qkv); add_img(P, b, e.mha.o); add_img(P, b, e.f1); add_img(P, b, e.f2); }
  for (const auto& e : L.dec) {
    add_img(P, b, e.mha1.qkv); add_img(P, b, e.mha1.o); add_img(P, b, e.mha2.q); add_img(P, b, e.mha2.kv); add_img(P, b, e.mha2.o);
    add_img(P, b, e.f1); add_img(P, b, e.f2);
  }
  add_img(P, b, L.bott_w); add_img(P, b, L.out);
  P.bytes = b.off;
  return P;
}

}  // namespace skf_model_detail
