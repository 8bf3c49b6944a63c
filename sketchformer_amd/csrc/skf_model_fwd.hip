// The fp32 forward: the fixed launch sequence of Transformer.call (models/sketchformer.py:131-181) up to the losses and metrics.
#include "skf_model_internal.h"

namespace skf_model_detail {

// classify_from_embedding (models/sketchformer.py:183-199): optional Dense(lowerdim, relu) + Dropout(class_dropout)
// buffers, then the classify layer -> logits in P.cls_logits (its softmax is fused into the CE kernel).
int classify_fwd(SkfModel* M, bool training, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan& P = M->plan;
  const float* fc = M->at<float>(P.emb);
  for (int i = 0; i < c.class_buffer_layers; ++i) {
    float* h = M->at<float>(P.cb_h[i]);
    float* fdrop = M->at<float>(P.cb_f[i]);
    SKF_TRY(dense_fwd(M, L.cbuf[i], fc, c.batch, h, 1, s));
    const float r = training ? c.class_dropout : 0.f;
    SKF_TRY(skf_dropout(h, fdrop, (size_t)c.batch * c.lowerdim, r, site_class(c.num_layers, i), M->state, s));
    fc = fdrop;
  }
  return dense_fwd(M, L.cls, fc, c.batch, M->at<float>(P.cls_logits), 0, s);
}

// The step metrics from the loss and hit sums of the two heads; absent heads contribute 0 rows: their loss is 0 in total_loss
// (sum(all_losses), models/sketchformer.py:345)
int metrics_update(SkfModel* M, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Plan& P = M->plan;
  const bool recon = do_recon(c);
  const float* recon_scalar = recon && c.continuous ? M->at<float>(P.cont_scal) + 3 : nullptr;
  return skf_metrics_update(M->at<float>(P.recon_loss), M->at<float>(P.recon_hit), recon ? c.batch * (c.seq_len - 1) : 0, c.recon_weight,
                            M->at<float>(P.cls_loss), M->at<float>(P.cls_hit), has_cls(c) ? c.batch : 0, c.class_weight, recon_scalar,
                            M->metrics, s);
}

namespace {
// The class cross-entropy of a step with a loss: loss and hit sums, probabilities, and d(logits) in place of the logits
int class_ce_with_grad(SkfModel* M, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Plan& P = M->plan;
  return skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, c.batch, c.n_classes, M->at<long long>(P.labels), 1, 1, 0, 0,
                        c.class_weight / (float)c.batch, M->at<float>(P.cls_loss), M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 1, s);
}

// The feed-forward block as one launch per direction (skf_ffn_fused.hip) where that kernel exists (d_model 128, dff 512, split
// arithmetic) unless SKF_MODEL_FFN_LAUNCHES asks for the separate launches.  Its pre-split weight images are rebuilt from the fp32
// masters at the start of every forward (one or two launches for all layers: whoever changed the weights - the optimizer, a
// checkpoint restore, a test - did not have to tell the library).
bool ffn_fused_on(const SkfModel* M) {
  const SkfConfig& c = M->cfg;
  return !(M->flags & SKF_MODEL_FFN_LAUNCHES) && skf_ffn_fused_supported(c.batch * c.seq_len, c.d_model, c.dff, c.gemm_precision) &&
         skf_ffn_image_bytes(c.d_model, c.dff, c.gemm_precision) > 0;
}
int build_ffn_images(SkfModel* M, bool with_backward, bool encoder_only, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan& P = M->plan;
  const int d = c.d_model, F = c.dff;
  const size_t half = skf_ffn_image_bytes(d, F, c.gemm_precision) / 2;
  std::vector<const float*> src; std::vector<int> ld, tr, K, N; std::vector<void*> img;
  auto one = [&](const DenseP& w, int t, int k, int n, char* im) {
    src.push_back(M->P(w.w)); ld.push_back(w.ld); tr.push_back(t); K.push_back(k); N.push_back(n); img.push_back(im);
  };
  auto ffn = [&](const DenseP& f1, const DenseP& f2, const size_t (&im)[2]) {
    one(f1, 0, d, F, M->at<char>(im[0])); one(f2, 0, F, d, M->at<char>(im[0]) + half);                  // forward: B1 = W1, B2 = W2
    if (with_backward) { one(f2, 1, d, F, M->at<char>(im[1])); one(f1, 1, F, d, M->at<char>(im[1]) + half); }   // backward: B1 = W2^T, B2 = W1^T
  };
  const bool dec = !encoder_only && do_recon(c);
  for (int i = 0; i < c.num_layers; ++i) {
    ffn(L.enc[i].f1, L.enc[i].f2, P.enc[i].img);
    if (i > 0) one(L.enc[i].mha.qkv, 0, d, 3 * d, M->at<char>(P.enc[i].img_qkv));
    one(L.enc[i].mha.o, 0, d, d, M->at<char>(P.enc[i].img_of));
    if (with_backward) one(L.enc[i].mha.o, 1, d, d, M->at<char>(P.enc[i].img_o));
  }
  if (dec)
    for (int i = 0; i < c.num_layers; ++i) {
      ffn(L.dec[i].f1, L.dec[i].f2, P.dec[i].img);
      if (i > 0) one(L.dec[i].mha1.qkv, 0, d, 3 * d, M->at<char>(P.dec[i].img_qkv));
      one(L.dec[i].mha2.o, 0, d, d, M->at<char>(P.dec[i].img_o2f));
      one(L.dec[i].mha1.o, 0, d, d, M->at<char>(P.dec[i].img_o1f)); one(L.dec[i].mha2.q, 0, d, d, M->at<char>(P.dec[i].img_q2));   // self-attention tail + query projection
      if (with_backward) { one(L.dec[i].mha1.o, 1, d, d, M->at<char>(P.dec[i].img_o1)); one(L.dec[i].mha2.o, 1, d, d, M->at<char>(P.dec[i].img_o2)); }
      if (with_backward) one(L.dec[i].mha2.q, 1, d, d, M->at<char>(P.dec[i].img_q2t));      // its input gradient rides in the self-attention sublayer's LayerNorm launch
    }
  return skf_dense_weight_images((int)src.size(), src.data(), ld.data(), tr.data(), K.data(), N.data(), img.data(), c.gemm_precision, s);
}
// The Dense that consumes a row-owner launch's output can be chained into that launch: d inputs, one of the projection widths the
// fused kernels are built for, dense rows
bool chains(const SkfModel* M, const DenseP& next) {
  return next.in == M->cfg.d_model && (next.out == 128 || next.out == 256 || next.out == 384) && next.ld == next.out;
}
// out = LayerNorm(x + dropout(ffn(x))): one launch, or Dense(relu) + Dense + residual-LayerNorm
// next / next_image / next_out: the Dense that consumes `out` (the next layer's q|k|v projection), taken into the same launch when
// the fused kernel runs (*next_done = true), else left to the caller
int ffn_ln_fwd(SkfModel* M, const DenseP& f1, const DenseP& f2, const LnP& ln, const float* x, int rows, float* h, void* bits,
               const void* image, float* z, float* out, float* stats, float rate, unsigned site, hipStream_t s,
               const DenseP* next = nullptr, const void* next_image = nullptr, float* next_out = nullptr, bool* next_done = nullptr) {
  const int d = M->cfg.d_model;
  if (next_done) *next_done = false;
  if (M->ctx.ffn_fused && next && chains(M, *next)) {
    if (next_done) *next_done = true;
    return skf_ffn_fused_fwd_proj_f32(rows, d, M->cfg.dff, x, image, M->P(f1.b), M->P(f2.b), h, bits, M->P(ln.g), M->P(ln.b), z, out, stats,
                                      rate, site, M->state, next_image, M->P(next->b), next->out, next_out, M->cfg.gemm_precision, s);
  }
  if (M->ctx.ffn_fused)
    return skf_ffn_fused_fwd_f32(rows, d, M->cfg.dff, x, image, M->P(f1.b), M->P(f2.b), h, bits, M->P(ln.g), M->P(ln.b), z, out, stats,
                                 rate, site, M->state, M->cfg.gemm_precision, s);
  SKF_TRY(dense_fwd_relu_bits(M, f1, x, rows, h, bits, s));
  SKF_TRY(dense_fwd(M, f2, h, rows, z, 0, s));
  return skf_layernorm_residual_fwd(x, z, M->P(ln.g), M->P(ln.b), out, stats, rows, d, rate, site, M->state, s);
}

// The tail of a layer behind its last attention: x1 = LayerNorm(x + dropout(o_proj(a))), out = LayerNorm(x1 + dropout(ffn(x1))) and,
// when there is one, the next layer's q|k|v projection - ONE launch (skf_ffn_block_fwd_f32) where the fused kernel runs, else the
// output-projection launch followed by ffn_ln_fwd.
int attn_tail_ffn_fwd(SkfModel* M, const DenseP& o, const LnP& ln_a, const float* a, const float* x, float* z1, float* x1, float* st1,
                      unsigned site_a, const void* o_image, const DenseP& f1, const DenseP& f2, const LnP& ln, float* h, void* bits,
                      const void* image, float* z, float* out, float* stats, unsigned site, int rows, float rate, hipStream_t s,
                      const DenseP* next, const void* next_image, float* next_out, bool* next_done) {
  const int d = M->cfg.d_model;
  if (!M->ctx.ffn_fused || o.in != d || o.out != d || ln_a.b != ln_a.g + (size_t)d) {
    SKF_TRY(dense_ln_fwd(M, o, a, rows, x, z1, ln_a, x1, st1, rate, site_a, s));
    return ffn_ln_fwd(M, f1, f2, ln, x1, rows, h, bits, image, z, out, stats, rate, site, s, next, next_image, next_out, next_done);
  }
  SkfFfnBlockFwd b{};
  b.struct_size = sizeof(SkfFfnBlockFwd); b.M = rows; b.d = d; b.dff = M->cfg.dff; b.precision = M->cfg.gemm_precision;
  b.x = a; b.image = image; b.b1 = M->P(f1.b); b.b2 = M->P(f2.b); b.h = h; b.relu_bits_out = bits;
  b.gamma = M->P(ln.g); b.beta = M->P(ln.b); b.z = z; b.out = out; b.stats = stats; b.rate = rate; b.site = site; b.step_state = M->state;
  b.pre_image = o_image; b.pre_bias = M->P(o.b); b.pre_residual = x; b.pre_gamma = M->P(ln_a.g); b.pre_beta = M->P(ln_a.b);
  b.pre_z = z1; b.pre_out = x1; b.pre_stats = st1; b.pre_site = site_a;
  const bool chain = next && chains(M, *next);
  if (chain) { b.proj_image = next_image; b.proj_bias = M->P(next->b); b.proj_out = next_out; b.proj_n = next->out; }
  if (next_done) *next_done = chain;
  return skf_ffn_block_fwd_f32(&b, s);
}

}  // namespace

// What the forward needs besides its inputs: the pre-split weight images of the row-owner launches (the weights changed in the last
// optimizer step), the two padding masks, and the samples sorted by length (both masks), longest first - every (sample, head)
// attention launch of the step deals its workgroups from that list.  None of it is read before the first attention.
int forward_preamble(SkfModel* M, bool with_backward, bool encoder_only, hipStream_t s, hipEvent_t masks_ready) {
  const SkfConfig& c = M->cfg;
  const Plan& P = M->plan;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1;
  unsigned char* emask = M->at<unsigned char>(P.enc_mask);
  unsigned char* dmask = M->at<unsigned char>(P.dec_mask);
  if (M->ctx.masks_staged) {
    // (written by the staging launch of this call)
  } else if (c.continuous) {
    SKF_TRY(skf_padding_mask_continuous(M->at<float>(P.inp), Le, B, Le, emask, s));
    SKF_TRY(skf_padding_mask_continuous(M->at<float>(P.tar), Le, B, Ld, dmask, s));
  } else {
    SKF_TRY(skf_padding_mask(M->at<long long>(P.inp), Le, B, Le, emask, s));
    SKF_TRY(skf_padding_mask(M->at<long long>(P.tar), Le, B, Ld, dmask, s));
  }
  M->ctx.order = nullptr;
  if (B <= 4096) {
    SKF_TRY(skf_sample_order(emask, Le, Le, encoder_only ? nullptr : dmask, Ld, Ld, B, M->at<int>(P.order), s));
    M->ctx.order = M->at<int>(P.order);
  }
  if (masks_ready) SKF_HIP(hipEventRecord(masks_ready, s));      // (the images are only read by the launch BEHIND the first attention)
  M->ctx.ffn_fused = ffn_fused_on(M);
  if (M->ctx.ffn_fused) SKF_TRY(build_ffn_images(M, with_backward, encoder_only, s));
  return SKF_OK;
}

int run_forward(SkfModel* M, bool training, bool with_loss, hipStream_t s, bool encoder_only) {
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan& P = M->plan;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1, d = c.d_model, H = c.num_heads, dh = d / H;
  const int Me = B * Le, Md = B * Ld, N = c.num_layers;
  const float rate = training ? c.dropout_rate : 0.f;
  const long long* inp = M->at<long long>(P.inp);
  const long long* tar = M->at<long long>(P.tar);
  unsigned char* emask = M->at<unsigned char>(P.enc_mask);
  unsigned char* dmask = M->at<unsigned char>(P.dec_mask);

  const float* inpf = M->at<float>(P.inp);      // continuous mode: (B, L, 5) stroke-5 rows
  const float* tarf = M->at<float>(P.tar);
  // weight images, padding masks, sample order: here, unless the train step already put them on the side stream (issue_embed_sorts)
  const hipEvent_t images_ready = M->ctx.pre_ready, masks_ready = M->ctx.masks_ready;
  if (!images_ready) SKF_TRY(forward_preamble(M, training && with_loss, encoder_only, s));
  const int* order = M->ctx.order;

  // ---------------- encoder (builders/layers/transformer.py:288-301)
  if (c.continuous)
    SKF_TRY(skf_embed_continuous_fwd(inpf, Le, B, Le, M->P(L.enc_embd.w), M->P(L.enc_embd.b), d, M->pos,
                                     M->at<float>(P.enc[0].x_in), rate, site_enc_embed(), M->state, s));
  else
    SKF_TRY(skf_embed_fwd(inp, Le, B, Le, M->P(L.enc_emb), c.vocab_size, d, M->pos, M->at<float>(P.enc[0].x_in), rate,
                          site_enc_embed(), M->state, s));
  bool enc_qkv_done = false;
  for (int i = 0; i < N; ++i) {
    const EncLayerP& w = L.enc[i];
    const EncAct& a = P.enc[i];
    float* x = M->at<float>(a.x_in);
    float* qkv = M->at<float>(a.qkv);
    if (!enc_qkv_done) SKF_TRY(dense_fwd(M, w.mha.qkv, x, Me, qkv, 0, s));     // (else: the previous layer's feed-forward launch wrote it)
    if (i == 0 && images_ready) SKF_HIP(hipStreamWaitEvent(s, masks_ready, 0));    // masks and order were built beside the embedding and this projection
    SKF_TRY(skf_attention_fwd_ordered(qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, emask, Le, 0, B, H, Le, Le, dh,
                                      M->at<float>(a.o), d, M->at<float>(a.astats), M->cfg.gemm_precision, order, s));
    const bool has_next = i + 1 < N;
    if (i == 0 && images_ready) SKF_HIP(hipStreamWaitEvent(s, images_ready, 0));      // ... and the weight images beside the first attention
    SKF_TRY(attn_tail_ffn_fwd(M, w.mha.o, w.ln1, M->at<float>(a.o), x, M->at<float>(a.z1), M->at<float>(a.x1), M->at<float>(a.st1),
                              site_enc(i, 0), M->at<char>(a.img_of), w.f1, w.f2, w.ln2, M->at<float>(a.h), hbits_of(M, a.hbits, Me),
                              M->at<char>(a.img[0]), M->at<float>(a.z2), M->at<float>(a.x2), M->at<float>(a.st2), site_enc(i, 1), Me, rate, s,
                              has_next ? &L.enc[i + 1].mha.qkv : nullptr, has_next ? M->at<char>(P.enc[i + 1].img_qkv) : nullptr,
                              has_next ? M->at<float>(P.enc[i + 1].qkv) : nullptr, &enc_qkv_done));
  }
  float* enc_out = M->at<float>(P.enc[N - 1].x2);
  // ---------------- bottleneck + classifier + expander (models/sketchformer.py:149-160,183-199,170-176)
  const int E = L.E, Ua = L.Ua;
  const bool bott = has_bott(c), cls = has_cls(c), recon = do_recon(c);
  if (bott) {
    SKF_TRY(dense_fwd(M, L.bott_w, enc_out, Me, M->at<float>(P.u), 2, s));
    SKF_TRY(skf_pool_fwd(M->at<float>(P.u), M->P(L.bott_v), enc_out, B, Le, Ua, d, M->at<float>(P.pool_a),
                         M->at<float>(c.attn_version == 2 ? P.pooled : P.emb), s));
    if (c.attn_version == 2)   // SelfAttnV2: o = embeding_layer(o) (builders/layers/transformer.py:128-129)
      SKF_TRY(dense_fwd(M, L.bott_e, M->at<float>(P.pooled), B, M->at<float>(P.emb), 0, s));
  }
  // The train step with a side stream and a decoder: the class head, its cross-entropy and the metrics launch have no main-stream
  // consumer before the classifier backward and go to the side stream (below).  Without a decoder there is no decoder-input event
  // and the side stream does nothing during the forward: the heads stay here, like everywhere without a side stream or a loss.
  const bool heads_on_side = with_loss && recon && M->sched.side;
  if (cls && !heads_on_side) SKF_TRY(classify_fwd(M, training, s));
  if (encoder_only || !recon) {
    if (encoder_only || !with_loss) {   // encode_from_seq / predict_class (models/sketchformer.py:162-168,223-228): class probabilities only
      if (!cls) return SKF_OK;
      return skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, B, c.n_classes, M->at<long long>(P.labels), 1, 1, 0, 0, 0.f,
                            M->at<float>(P.cls_loss), M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 0, s);
    }
  }
  // pre_decoder: the expanded embedding, or the encoder output itself when there is no bottleneck (:172-176)
  float* pre = bott ? M->at<float>(P.pre) : enc_out;
  // pre_decoder is all the side stream's cross-attention K|V projections wait for: their event rides on the expander launch
  hipEvent_t dec_in_ready = nullptr;
  bool dec_in_recorded = false;
  if (recon && M->sched.side) {
    M->sched.rewind_events();      // (the step's earlier events - masks, images - were waited for in front of the first encoder layer)
    dec_in_ready = M->sched.take_event();
    SKF_CHECK_ARG(dec_in_ready, "event allocation failed");
  }
  if (recon && bott) {
    SKF_TRY(with_tail_event(M, dec_in_ready, &dec_in_recorded,
                            [&] { return skf_expander_fwd(M->at<float>(P.emb), M->P(L.exp_w), M->P(L.exp_b), B, Le, E, pre, s); }));
  }

  // ---------------- decoder (builders/layers/transformer.py:325-344)
  if (recon) {
  if (c.continuous)
    SKF_TRY(skf_embed_continuous_fwd(tarf, Le, B, Ld, M->P(L.dec_embd.w), M->P(L.dec_embd.b), d, M->pos,
                                     M->at<float>(P.dec[0].x_in), rate, site_dec_embed(N), M->state, s));
  else
    SKF_TRY(skf_embed_fwd(tar, Le, B, Ld, M->P(L.dec_emb), c.vocab_size, d, M->pos, M->at<float>(P.dec[0].x_in), rate,
                          site_dec_embed(N), M->state, s));
  const unsigned char* cross_mask = c.blind_decoder_mask ? nullptr : emask;
  // The cross-attention K|V projections of ALL decoder layers only depend on pre_decoder: on the eager path they run
  // on the side stream under the first layer's self-attention block (one event pair) instead of on the critical path.
  // (round 5: the first layer's cross-attention waits for ITS projection only - it used to wait for all of them, 45 us with the main
  //  stream idle at cfg 2 - the second layer's for the rest)
  hipEvent_t kv_done = nullptr, kv_first = nullptr;
  if (M->sched.side) {
    kv_done = M->sched.take_event();
    kv_first = N > 1 ? M->sched.take_event() : kv_done;
    SKF_CHECK_ARG(dec_in_ready && kv_done && kv_first, "event allocation failed");
    if (!dec_in_recorded) SKF_HIP(hipEventRecord(dec_in_ready, s));
    SKF_HIP(hipStreamWaitEvent(M->sched.side, dec_in_ready, 0));
    // The class head and its cross-entropy (train step): dec_in_ready rides on the expander launch (or is recorded above), which
    // follows the pooling / embedding launches on the main stream, so the embedding is visible behind this wait.  In FRONT of the K|V
    // projections, not behind the first one: the two launches take ~21 us and the first projection then still ends ~50 us before the
    // first cross-attention asks for it (profiles/side_stream_moves_ab.txt), and this way one argument orders the main stream's
    // readers in every structure - the main stream waits for kv_first (recorded below, behind these launches on the in-order side
    // stream) in front of the first layer's cross-attention, one layer included, long before the classifier backward reads dcls, the
    // class-buffer activations, cls_loss or cls_hit.  What they overwrite belongs to the previous step, whose final join put both
    // streams behind its last reader.
    if (cls && heads_on_side) {
      SKF_TRY(classify_fwd(M, training, M->sched.side));
      SKF_TRY(class_ce_with_grad(M, M->sched.side));
    }
    for (int i = 0; i < N; ++i) {
      SKF_TRY(dense_fwd(M, L.dec[i].mha2.kv, pre, Me, M->at<float>(P.dec[i].kv2), 0, M->sched.side));
      if (i == 0 && kv_first != kv_done) SKF_HIP(hipEventRecord(kv_first, M->sched.side));
    }
    SKF_HIP(hipEventRecord(kv_done, M->sched.side));
  }
  bool dec_qkv_done = false;
  for (int i = 0; i < N; ++i) {
    const DecLayerP& w = L.dec[i];
    const DecAct& a = P.dec[i];
    float* x = M->at<float>(a.x_in);
    float* qkv = M->at<float>(a.qkv);
    if (!dec_qkv_done) SKF_TRY(dense_fwd(M, w.mha1.qkv, x, Md, qkv, 0, s));
    SKF_TRY(skf_attention_fwd_ordered(qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, dmask, Ld, 1, B, H, Ld, Ld, dh,
                                      M->at<float>(a.o1), d, M->at<float>(a.astats1), M->cfg.gemm_precision, order, s));
    // out1 = LayerNorm(x + dropout(o1 . Wo + bo)) and q2 = out1 . Wq + bq: one row-owner launch where that kernel runs
    // (skf_ffn_block_fwd_f32 without a feed-forward image), else the fused Dense + LayerNorm launch and the projection launch
    const bool tail_proj = M->ctx.ffn_fused && w.mha1.o.in == d && w.mha1.o.out == d && chains(M, w.mha2.q) && w.mha2.q.out == d &&
                           w.ln1.b == w.ln1.g + (size_t)d;
    if (tail_proj) {
      SkfFfnBlockFwd tb{};
      tb.struct_size = sizeof(SkfFfnBlockFwd); tb.M = Md; tb.d = d; tb.dff = c.dff; tb.precision = c.gemm_precision;
      tb.x = M->at<float>(a.o1); tb.rate = rate; tb.step_state = M->state;
      tb.pre_image = M->at<char>(a.img_o1f); tb.pre_bias = M->P(w.mha1.o.b); tb.pre_residual = x; tb.pre_gamma = M->P(w.ln1.g); tb.pre_beta = M->P(w.ln1.b);
      tb.pre_z = M->at<float>(a.z1); tb.pre_out = M->at<float>(a.out1); tb.pre_stats = M->at<float>(a.st1); tb.pre_site = site_dec(N, i, 0);
      tb.proj_image = M->at<char>(a.img_q2); tb.proj_bias = M->P(w.mha2.q.b); tb.proj_out = M->at<float>(a.q2); tb.proj_n = d;
      SKF_TRY(skf_ffn_block_fwd_f32(&tb, s));
    } else {
      SKF_TRY(dense_ln_fwd(M, w.mha1.o, M->at<float>(a.o1), Md, x, M->at<float>(a.z1), w.ln1, M->at<float>(a.out1), M->at<float>(a.st1),
                           rate, site_dec(N, i, 0), s));
      SKF_TRY(dense_fwd(M, w.mha2.q, M->at<float>(a.out1), Md, M->at<float>(a.q2), 0, s));
    }
    float* kv2 = M->at<float>(a.kv2);
    if (!kv_done) SKF_TRY(dense_fwd(M, w.mha2.kv, pre, Me, kv2, 0, s));
    else if (i == 0) SKF_HIP(hipStreamWaitEvent(s, kv_first, 0));
    else if (i == 1) SKF_HIP(hipStreamWaitEvent(s, kv_done, 0));
    SKF_TRY(skf_attention_fwd_ordered(M->at<float>(a.q2), d, kv2, 2 * d, kv2 + d, 2 * d, cross_mask, Le, 0, B, H, Ld, Le, dh,
                                      M->at<float>(a.o2), d, M->at<float>(a.astats2), M->cfg.gemm_precision, order, s));
    const bool has_next = i + 1 < N;
    SKF_TRY(attn_tail_ffn_fwd(M, w.mha2.o, w.ln2, M->at<float>(a.o2), M->at<float>(a.out1), M->at<float>(a.z2), M->at<float>(a.out2),
                              M->at<float>(a.st2), site_dec(N, i, 1), M->at<char>(a.img_o2f), w.f1, w.f2, w.ln3, M->at<float>(a.h),
                              hbits_of(M, a.hbits, Md), M->at<char>(a.img[0]), M->at<float>(a.z3), M->at<float>(a.out3), M->at<float>(a.st3),
                              site_dec(N, i, 2), Md, rate, s, has_next ? &L.dec[i + 1].mha1.qkv : nullptr,
                              has_next ? M->at<char>(P.dec[i + 1].img_qkv) : nullptr, has_next ? M->at<float>(P.dec[i + 1].qkv) : nullptr,
                              &dec_qkv_done));
  }
  SKF_TRY(dense_fwd(M, L.out, M->at<float>(P.dec[N - 1].out3), Md, M->at<float>(P.logits), 0, s));
  }

  // ---------------- losses + metrics (models/sketchformer.py:334-346)
  const long long* labels = M->at<long long>(P.labels);
  if (with_loss) {
    // tar_real = tar[:, 1:]  -> target offset 1 within rows of stride L
    if (recon) {
      if (c.continuous) {
        SKF_TRY(skf_continuous_loss(M->at<float>(P.logits), tarf, Le, Ld, 1, Md, c.recon_weight, M->at<float>(P.recon_loss),
                                    M->at<float>(P.recon_hit), M->at<float>(P.row_mask), M->at<float>(P.cont_scal), 1, s));
      } else {
        SKF_TRY(skf_softmax_ce(M->at<float>(P.logits), c.vocab_size, Md, c.vocab_size, tar, Le, Ld, 1, 1,
                               c.recon_weight / (float)Md, M->at<float>(P.recon_loss), M->at<float>(P.recon_hit), nullptr, 1, s));
      }
    }
    if (cls && !heads_on_side) SKF_TRY(class_ce_with_grad(M, s));
    // (two streams: run_backward issues it on the side stream, behind the first wait that orders that stream after the token loss)
    if (heads_on_side) M->ctx.metrics_deferred = true;
    else SKF_TRY(metrics_update(M, s));
  } else if (cls) {
    SKF_TRY(skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, B, c.n_classes, labels, 1, 1, 0, 0, 0.f,
                           M->at<float>(P.cls_loss), M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 0, s));
  }
  return SKF_OK;
}

}  // namespace skf_model_detail
