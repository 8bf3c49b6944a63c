// bf16 path of the train-step orchestrator (BASELINE cfg 5); its workspace plan is build_plan16 (skf_model_layout.hip).
//
// The same launch sequence as run_forward / run_backward (models/sketchformer.py:131-181, 325-349) with bf16 activations:
// Dense layers on skf_gemm_bf16 / skf_gemm_bf16_wgrad, attention on the streaming kernels, row stages on the *_bf16 row
// kernels.  Parameters, gradients and optimizer state stay the flat fp32 buffers of the fp32 path (same layout, same names);
// every forward first refreshes the bf16 images of the Dense weights ([in][out] for the input gradients, [out][in] for the
// forward) from the fp32 masters, so that a caller may edit the masters at any time.  The small per-sample heads (classifier,
// its loss) run on the fp32 kernels.  One stream, weight gradients in line (partial tiles + their reduction), two gradient
// buckets like the fp32 path.  Structure restrictions (skf_config_validate): token mode, attn_version 1, bottleneck +
// classifier + decoder, no class buffers, head size 64.
#include "skf_model_internal.h"

namespace skf_model_detail {
namespace {

inline void* w16(SkfModel* M, size_t off) { return M->ws + off; }

}  // namespace

// the named activations of the bf16 plan (bf16 unless said otherwise: row pitch `ld` elements)
void register_buffers16(SkfModel* M) {
  const SkfConfig& c = M->cfg;
  const Plan16& P = M->p16;
  const size_t B = c.batch, Ls = c.seq_len, d = c.d_model, F = c.dff, Me = B * Ls, Md = B * (Ls - 1), N = c.num_layers;
  M->reg("logits", P.logits, Md, c.vocab_size, P.ld_logits, 1);
  M->reg("class_probs", P.cls_probs, B, c.n_classes, c.n_classes, 0);
  M->reg("class_logits", P.cls_logits, B, c.n_classes, c.n_classes, 0);
  M->reg("embedding", P.emb, B, d, d, 0);
  M->reg("enc_output", P.enc[N - 1].x2, Me, d, d, 1);
  M->reg("dec_output", P.dec[N - 1].out3, Md, d, d, 1);
  M->reg("pre_decoder", P.pre, Me, d, d, 1);
  M->reg("bottleneck_attn", P.pool_a, B, Ls, Ls, 0);
  M->reg("enc_embed_out", P.enc[0].x_in, Me, d, d, 1);
  M->reg("dec_embed_out", P.dec[0].x_in, Md, d, d, 1);
  for (size_t i = 0; i < N; ++i) {
    M->reg("encoder/layer" + std::to_string(i) + "/ffn_h", P.enc[i].h, Me, F, F, 1);
    M->reg("decoder/layer" + std::to_string(i) + "/ffn_h", P.dec[i].h, Md, F, F, 1);
  }
}

// descriptor table of the weight images, uploaded once per binding of the parameter buffer (outside any graph capture:
// every call builds it in front of its staging copies, stage_batch)
int ensure_cast_table16(SkfModel* M, hipStream_t s) {
  Plan16& P = M->p16;
  if (P.cast_for == M->params && P.tables_ws == M->ws) return SKF_OK;
  std::vector<SkfCastDesc> descs;
  int blocks = 0;
  for (const auto& kv : P.img) {
    const Img16& im = kv.second;
    SkfCastDesc d{};
    d.src = M->P(im.src); d.dst = w16(M, im.w); d.dst_t = w16(M, im.wt);
    d.R = im.in; d.C = im.out; d.ld_src = im.ld_src; d.ld_dst = im.ldw; d.ld_t = im.ldt; d.block_begin = blocks;
    int bx = 0;
    blocks += skf_cast_weight_bf16_blocks(im.in, im.out, im.ldw, im.ldt, &bx);
    d.blocks_x = bx;
    descs.push_back(d);
  }
  SKF_CHECK_ARG(descs.size() * sizeof(SkfCastDesc) <= P.cast_descs_bytes, "image descriptor table too small");
  SKF_HIP(hipStreamSynchronize(s));                      // (a step in flight may still read the old table)
  SKF_HIP(hipMemcpy(M->ws + P.cast_descs, descs.data(), descs.size() * sizeof(SkfCastDesc), hipMemcpyHostToDevice));
  P.cast_n = (int)descs.size(); P.cast_blocks = blocks; P.cast_for = M->params; P.tables_ws = M->ws;
  // LayerNorm partial slabs in the order run_backward16 visits them: decoder layers N-1..0 (ln3, ln2, ln1), encoder layers
  // N-1..0 (ln2, ln1); a slab is "g splits of a 1 x 2d matrix" for the batched split-K reduction (gamma and beta adjacent)
  {
    const SkfConfig& c = M->cfg;
    const Layout& L = M->lay;
    const int N = c.num_layers, d = c.d_model;
    const int Me = c.batch * c.seq_len, Md = c.batch * (c.seq_len - 1);
    std::vector<SkfReduceDesc> rd;
    bool adjacent = true;
    int blocks_run = 0;
    auto add = [&](const LnP& ln, int rows) {
      SkfReduceDesc q{};
      q.slab = reinterpret_cast<const float*>(M->ws + P.ln_slabs + rd.size() * P.ln_ws_bytes);
      q.C = M->G(ln.g); q.bias_grad = nullptr; q.M = 1; q.N = 2 * d; q.ldc = 2 * d;
      q.splits = (int)(skf_layernorm_bwd_bf16_workspace_bytes(rows, d) / ((size_t)8 * d));
      q.block_begin = blocks_run; q.pad = 0;
      blocks_run += skf_splitk_reduce_blocks(1, 2 * d);
      adjacent = adjacent && ln.b == ln.g + (size_t)d;
      rd.push_back(q);
    };
    for (int i = N - 1; i >= 0; --i) { add(L.dec[i].ln3, Md); add(L.dec[i].ln2, Md); add(L.dec[i].ln1, Md); }
    P.ln_blocks_dec = blocks_run;
    blocks_run = 0;
    for (int i = N - 1; i >= 0; --i) { add(L.enc[i].ln2, Me); add(L.enc[i].ln1, Me); }
    P.ln_blocks_enc = blocks_run;
    P.ln_batched = adjacent && (int)rd.size() == P.ln_n;
    if (P.ln_batched) SKF_HIP(hipMemcpy(M->ws + P.ln_descs, rd.data(), rd.size() * sizeof(SkfReduceDesc), hipMemcpyHostToDevice));
  }
  return SKF_OK;
}
namespace {
int refresh_images16(SkfModel* M, hipStream_t s) {
  SkfProfScope ps(s, "weight_images_bf16", 0.0, 0.0);
  const Plan16& P = M->p16;
  SKF_CHECK_ARG(P.cast_for == M->params && P.tables_ws == M->ws, "weight-image table not built (the staging of a call does it)");
  return skf_cast_weight_bf16_batch(reinterpret_cast<const SkfCastDesc*>(M->ws + P.cast_descs), P.cast_n, P.cast_blocks, s);
}
// y[rows][w.out] = x . W + b (act)
int d16_fwd(SkfModel* M, const DenseP& w, const void* x, int ldx, int rows, void* y, int ldy, int act, hipStream_t s) {
  const Img16& im = M->p16.img.at(w.w);
  return skf_gemm_bf16(rows, w.out, w.in, x, ldx, w16(M, im.wt), im.ldt, y, ldy, M->P(w.b), act, nullptr, 0, 0, nullptr, 0, s);
}
// sign-bit buffer of an ffn hidden tensor, or null (dff % 8 != 0)
void* hbits16(SkfModel* M, size_t off) {
  return (M->cfg.dff & 7) ? nullptr : M->ws + off;
}
// ffn dense1: relu forward that also leaves the sign bits of the hidden tensor
int d16_fwd_relu_bits(SkfModel* M, const DenseP& w, const void* x, int ldx, int rows, void* y, int ldy, void* bits, hipStream_t s) {
  const Img16& im = M->p16.img.at(w.w);
  return skf_gemm_bf16_bits(rows, w.out, w.in, x, ldx, w16(M, im.wt), im.ldt, y, ldy, M->P(w.b), 1, nullptr, 0, 0, nullptr, 0, nullptr, 0,
                            bits, nullptr, w.out >> 3, s);
}
// dx[rows][w.in] (+)= dy . W^T (o relu mask)
// Problems with exactly as many rows as the live lists cover (the decoder side, while StepCtx has them set) run over the live rows
// (dgrad: tiles of the compacted row list) / live 64-row blocks (weight gradient).  Dead output rows are always zero-filled: readers that
// do not walk the lists (the 128 x 128 weight-gradient kernel, LayerNorm, attention) see every row.
int d16_dgrad(SkfModel* M, const DenseP& w, const void* dy, int lddy, int rows, void* dx, int lddx, int accumulate,
              const void* relu_src, int ld_relu, hipStream_t s, const void* relu_bits = nullptr) {
  const int zero_dead = 1;
  const Img16& im = M->p16.img.at(w.w);
  return skf_gemm_bf16_bits(rows, w.in, w.out, dy, lddy, w16(M, im.w), im.ldw, dx, lddx, nullptr, 0, relu_bits ? nullptr : relu_src, ld_relu,
                            accumulate, nullptr, 0, M->ctx.live_blocks(rows, 1), zero_dead, nullptr, relu_bits, w.in >> 3, s);
}
int d16_wgrad(SkfModel* M, const DenseP& w, const void* x, int ldx, const void* dy, int lddy, int rows, hipStream_t s) {
  return skf_gemm_bf16_wgrad_rows(w.in, w.out, rows, x, ldx, dy, lddy, M->G(w.w), w.ld, M->G(w.b), w16(M, M->p16.slab), M->p16.slab_bytes,
                                  M->ctx.live_blocks(rows, 64), s);
}
int ln16_fwd(SkfModel* M, const LnP& ln, const void* x, void* y_z, void* out, size_t st, int rows, float rate, unsigned site, hipStream_t s) {
  return skf_layernorm_residual_fwd_bf16(x, y_z, M->P(ln.g), M->P(ln.b), out, M->at<float>(st), rows, M->cfg.d_model, rate, site, M->state, s);
}
int ln16_bwd(SkfModel* M, const LnP& ln, const void* dout, size_t z, size_t st, void* dz, void* dy, int rows, float rate, unsigned site,
             hipStream_t s) {
  Plan16& P = M->p16;
  const int* ll = M->ctx.live_lengths(rows);       // decoder side of a padded batch: dead rows are stored as zeros
  if (P.ln_batched) {
    // partials only, into this call's slab; ln16_reduce() sums a whole side's slabs in one launch
    SKF_CHECK_ARG(P.ln_cursor < P.ln_n, "more LayerNorm backward calls than slabs");
    char* slab = M->ws + P.ln_slabs + (size_t)P.ln_cursor++ * P.ln_ws_bytes;
    return skf_layernorm_residual_bwd_bf16_rows(dout, w16(M, z), M->at<float>(st), M->P(ln.g), dz, dy, nullptr, nullptr, rows, M->cfg.d_model,
                                                rate, site, M->state, slab, P.ln_ws_bytes, ll, M->cfg.seq_len - 1, s);
  }
  return skf_layernorm_residual_bwd_bf16_rows(dout, w16(M, z), M->at<float>(st), M->P(ln.g), dz, dy, M->G(ln.g), M->G(ln.b), rows,
                                              M->cfg.d_model, rate, site, M->state, w16(M, P.ln_ws), P.ln_ws_bytes, ll, M->cfg.seq_len - 1, s);
}
// gamma / beta gradients of the decoder-side (first = true) or encoder-side LayerNorms from their partial slabs
int ln16_reduce(SkfModel* M, bool first, hipStream_t s) {
  const Plan16& P = M->p16;
  if (!P.ln_batched) return SKF_OK;
  const SkfReduceDesc* descs = reinterpret_cast<const SkfReduceDesc*>(M->ws + P.ln_descs);
  if (first) return skf_splitk_reduce_batch(descs, P.ln_n_dec, P.ln_blocks_dec, s);
  return skf_splitk_reduce_batch(descs + P.ln_n_dec, P.ln_n - P.ln_n_dec, P.ln_blocks_enc, s);
}

}  // namespace
int run_forward16(SkfModel* M, bool training, bool with_loss, hipStream_t s, bool encoder_only) {
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan16& P = M->p16;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1, d = c.d_model, H = c.num_heads, dh = d / H, F = c.dff, U = c.lowerdim;
  const int Me = B * Le, Md = B * Ld, N = c.num_layers;
  const float rate = training ? c.dropout_rate : 0.f;
  const long long* inp = M->at<long long>(P.inp);
  const long long* tar = M->at<long long>(P.tar);
  unsigned char* emask = M->at<unsigned char>(P.enc_mask);
  unsigned char* dmask = M->at<unsigned char>(P.dec_mask);
  char* W = M->ws;
  SKF_TRY(refresh_images16(M, s));
  SKF_TRY(skf_padding_mask(inp, Le, B, Le, emask, s));
  SKF_TRY(skf_padding_mask(tar, Le, B, Ld, dmask, s));
  // samples by length, longest first: the attention launches deal their workgroups over XCDs and shader engines from it
  M->ctx.order = nullptr;
  if (B <= 4096) {
    SKF_TRY(skf_sample_order(emask, Le, Le, encoder_only ? nullptr : dmask, Ld, Ld, B, M->at<int>(P.order), s));
    M->ctx.order = M->at<int>(P.order);
  }
  const int* order = M->ctx.order;
  // ---------------- encoder
  SKF_TRY(skf_embed_fwd_bf16(inp, Le, B, Le, M->P(L.enc_emb), c.vocab_size, d, M->pos, W + P.enc[0].x_in, rate, site_enc_embed(), M->state, s));
  for (int i = 0; i < N; ++i) {
    const EncLayerP& w = L.enc[i];
    const Enc16& a = P.enc[i];
    char* qkv = W + a.qkv;
    SKF_TRY(d16_fwd(M, w.mha.qkv, W + a.x_in, d, Me, qkv, 3 * d, 0, s));
    SKF_TRY(skf_attention_bf16_fwd_ordered(qkv, 3 * d, qkv + 2 * d, 3 * d, qkv + 4 * d, 3 * d, emask, Le, 0, B, H, Le, Le, dh, W + a.o, d,
                                   W + a.olo, M->at<float>(a.astats), order, s));
    SKF_TRY(d16_fwd(M, w.mha.o, W + a.o, d, Me, W + a.z1, d, 0, s));
    SKF_TRY(ln16_fwd(M, w.ln1, W + a.x_in, W + a.z1, W + a.x1, a.st1, Me, rate, site_enc(i, 0), s));
    SKF_TRY(d16_fwd_relu_bits(M, w.f1, W + a.x1, d, Me, W + a.h, F, hbits16(M, a.hbits), s));
    SKF_TRY(d16_fwd(M, w.f2, W + a.h, F, Me, W + a.z2, d, 0, s));
    SKF_TRY(ln16_fwd(M, w.ln2, W + a.x1, W + a.z2, W + a.x2, a.st2, Me, rate, site_enc(i, 1), s));
  }
  char* enc_out = W + P.enc[N - 1].x2;
  // ---------------- bottleneck, classifier (fp32 head), expander
  SKF_TRY(d16_fwd(M, L.bott_w, enc_out, d, Me, W + P.u, U, 2, s));
  SKF_TRY(skf_pool_fwd_bf16(W + P.u, M->P(L.bott_v), enc_out, B, Le, U, d, M->at<float>(P.pool_a), M->at<float>(P.emb), s));
  SKF_TRY(skf_gemm_f32(1, 0, B, c.n_classes, d, M->at<float>(P.emb), d, M->P(L.cls.w), L.cls.ld, M->at<float>(P.cls_logits), c.n_classes,
                       M->P(L.cls.b), 0, nullptr, 0, 0, 1, nullptr, 0, nullptr, 0, SKF_PREC_F32, s));
  const long long* labels = M->at<long long>(P.labels);
  if (encoder_only)
    return skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, B, c.n_classes, labels, 1, 1, 0, 0, 0.f, M->at<float>(P.cls_loss),
                          M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 0, s);
  SKF_TRY(skf_expander_fwd_bf16(M->at<float>(P.emb), M->P(L.exp_w), M->P(L.exp_b), B, Le, d, W + P.pre, s));
  // ---------------- decoder
  SKF_TRY(skf_embed_fwd_bf16(tar, Le, B, Ld, M->P(L.dec_emb), c.vocab_size, d, M->pos, W + P.dec[0].x_in, rate, site_dec_embed(N), M->state, s));
  const unsigned char* cross_mask = c.blind_decoder_mask ? nullptr : emask;
  for (int i = 0; i < N; ++i) {
    const DecLayerP& w = L.dec[i];
    const Dec16& a = P.dec[i];
    char* qkv = W + a.qkv;
    char* kv2 = W + a.kv2;
    SKF_TRY(d16_fwd(M, w.mha1.qkv, W + a.x_in, d, Md, qkv, 3 * d, 0, s));
    SKF_TRY(skf_attention_bf16_fwd_ordered(qkv, 3 * d, qkv + 2 * d, 3 * d, qkv + 4 * d, 3 * d, dmask, Ld, 1, B, H, Ld, Ld, dh, W + a.o1, d,
                                   W + a.olo1, M->at<float>(a.astats1), order, s));
    SKF_TRY(d16_fwd(M, w.mha1.o, W + a.o1, d, Md, W + a.z1, d, 0, s));
    SKF_TRY(ln16_fwd(M, w.ln1, W + a.x_in, W + a.z1, W + a.out1, a.st1, Md, rate, site_dec(N, i, 0), s));
    SKF_TRY(d16_fwd(M, w.mha2.q, W + a.out1, d, Md, W + a.q2, d, 0, s));
    SKF_TRY(d16_fwd(M, w.mha2.kv, W + P.pre, d, Me, kv2, 2 * d, 0, s));
    SKF_TRY(skf_attention_bf16_fwd_ordered(W + a.q2, d, kv2, 2 * d, kv2 + 2 * d, 2 * d, cross_mask, Le, 0, B, H, Ld, Le, dh, W + a.o2, d,
                                   W + a.olo2, M->at<float>(a.astats2), order, s));
    SKF_TRY(d16_fwd(M, w.mha2.o, W + a.o2, d, Md, W + a.z2, d, 0, s));
    SKF_TRY(ln16_fwd(M, w.ln2, W + a.out1, W + a.z2, W + a.out2, a.st2, Md, rate, site_dec(N, i, 1), s));
    SKF_TRY(d16_fwd_relu_bits(M, w.f1, W + a.out2, d, Md, W + a.h, F, hbits16(M, a.hbits), s));
    SKF_TRY(d16_fwd(M, w.f2, W + a.h, F, Md, W + a.z3, d, 0, s));
    SKF_TRY(ln16_fwd(M, w.ln3, W + a.out2, W + a.z3, W + a.out3, a.st3, Md, rate, site_dec(N, i, 2), s));
  }
  SKF_TRY(d16_fwd(M, L.out, W + P.dec[N - 1].out3, d, Md, W + P.logits, P.ld_logits, 0, s));
  // ---------------- losses + metrics
  if (with_loss) {
    SKF_TRY(skf_softmax_ce_bf16(W + P.logits, P.ld_logits, Md, c.vocab_size, tar, Le, Ld, 1, 1, c.recon_weight / (float)Md,
                                M->at<float>(P.recon_loss), M->at<float>(P.recon_hit), 1, s));
    SKF_TRY(skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, B, c.n_classes, labels, 1, 1, 0, 0, c.class_weight / (float)B,
                           M->at<float>(P.cls_loss), M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 1, s));
    SKF_TRY(skf_metrics_update(M->at<float>(P.recon_loss), M->at<float>(P.recon_hit), Md, c.recon_weight, M->at<float>(P.cls_loss),
                               M->at<float>(P.cls_hit), B, c.class_weight, nullptr, M->metrics, s));
  } else {
    SKF_TRY(skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, B, c.n_classes, labels, 1, 1, 0, 0, 0.f, M->at<float>(P.cls_loss),
                           M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 0, s));
  }
  return SKF_OK;
}

int run_backward16(SkfModel* M, hipStream_t s) {
  M->ctx.begin_backward();      // stale state of a backward that returned early must not reach this one
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan16& P = M->p16;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1, d = c.d_model, H = c.num_heads, dh = d / H, F = c.dff, U = c.lowerdim;
  const int Me = B * Le, Md = B * Ld, N = c.num_layers;
  const float rate = c.dropout_rate;
  const unsigned char* emask = M->at<unsigned char>(P.enc_mask);
  const unsigned char* dmask = M->at<unsigned char>(P.dec_mask);
  char* W = M->ws;
  char* G = W + P.gA;
  char* G2 = W + P.gB;
  char* dy = W + P.dy;
  char* dO = W + P.dO;
  char* dqkv = W + P.dqkv;
  char* dhb = W + P.dh;
  char* dpre = W + P.dpre;
  char* dkv2 = W + P.dkv2;
  char* dq2 = W + P.dq2;
  float* demb = M->at<float>(P.demb);
  void* aws = W + P.attn_ws;
  M->p16.ln_cursor = 0;
  // ---------------- decoder side: every (B * Ld)-row gradient is zero behind a sample's last trained position (skf_row_blocks.hip)
  int* ll = M->at<int>(P.live_len);
  SKF_TRY(skf_target_live_len(M->at<long long>(P.tar), Le, B, Ld, ll, s));
  SKF_TRY(skf_row_blocks_build(ll, B, Ld, 1, M->at<int>(P.live1), s));
  SKF_TRY(skf_row_blocks_build(ll, B, Ld, 64, M->at<int>(P.live64), s));
  M->ctx.set_live(Md, ll, 1, M->at<int>(P.live1), 64, M->at<int>(P.live64));
  // ---------------- output layer (the logits buffer holds dlogits, pad columns zero)
  SKF_TRY(d16_wgrad(M, L.out, W + P.dec[N - 1].out3, d, W + P.logits, P.ld_logits, Md, s));
  SKF_TRY(d16_dgrad(M, L.out, W + P.logits, P.ld_logits, Md, G, d, 0, nullptr, 0, s));
  const unsigned char* cross_mask = c.blind_decoder_mask ? nullptr : emask;
  for (int i = N - 1; i >= 0; --i) {
    const DecLayerP& w = L.dec[i];
    const Dec16& a = P.dec[i];
    SKF_TRY(ln16_bwd(M, w.ln3, G, a.z3, a.st3, G2, dy, Md, rate, site_dec(N, i, 2), s));
    SKF_TRY(d16_wgrad(M, w.f2, W + a.h, F, dy, d, Md, s));
    SKF_TRY(d16_dgrad(M, w.f2, dy, d, Md, dhb, F, 0, W + a.h, F, s, hbits16(M, a.hbits)));
    SKF_TRY(d16_wgrad(M, w.f1, W + a.out2, d, dhb, F, Md, s));
    SKF_TRY(d16_dgrad(M, w.f1, dhb, F, Md, G2, d, 1, nullptr, 0, s));
    SKF_TRY(ln16_bwd(M, w.ln2, G2, a.z2, a.st2, G, dy, Md, rate, site_dec(N, i, 1), s));
    SKF_TRY(d16_wgrad(M, w.mha2.o, W + a.o2, d, dy, d, Md, s));
    SKF_TRY(d16_dgrad(M, w.mha2.o, dy, d, Md, dO, d, 0, nullptr, 0, s));
    const char* kv2 = W + a.kv2;
    const int* qlive = M->ctx.live_lengths(Md);      // decoder query rows behind it have dO == 0
    SKF_TRY(skf_attention_bf16_bwd_ordered(W + a.q2, d, kv2, 2 * d, kv2 + 2 * d, 2 * d, W + a.o2, d, W + a.olo2, dO, d, M->at<float>(a.astats2), cross_mask,
                                        Le, 0, B, H, Ld, Le, dh, dq2, d, dkv2, 2 * d, dkv2 + 2 * d, 2 * d, aws, P.attn_ws_bytes, qlive, M->ctx.order, s));
    SKF_TRY(d16_wgrad(M, w.mha2.q, W + a.out1, d, dq2, d, Md, s));
    SKF_TRY(d16_dgrad(M, w.mha2.q, dq2, d, Md, G, d, 1, nullptr, 0, s));
    SKF_TRY(d16_wgrad(M, w.mha2.kv, W + P.pre, d, dkv2, 2 * d, Me, s));
    SKF_TRY(d16_dgrad(M, w.mha2.kv, dkv2, 2 * d, Me, dpre, d, i != N - 1, nullptr, 0, s));
    SKF_TRY(ln16_bwd(M, w.ln1, G, a.z1, a.st1, G2, dy, Md, rate, site_dec(N, i, 0), s));
    SKF_TRY(d16_wgrad(M, w.mha1.o, W + a.o1, d, dy, d, Md, s));
    SKF_TRY(d16_dgrad(M, w.mha1.o, dy, d, Md, dO, d, 0, nullptr, 0, s));
    const char* qkv = W + a.qkv;
    SKF_TRY(skf_attention_bf16_bwd_ordered(qkv, 3 * d, qkv + 2 * d, 3 * d, qkv + 4 * d, 3 * d, W + a.o1, d, W + a.olo1, dO, d, M->at<float>(a.astats1), dmask, Ld,
                                        1, B, H, Ld, Ld, dh, dqkv, 3 * d, dqkv + 2 * d, 3 * d, dqkv + 4 * d, 3 * d, aws, P.attn_ws_bytes, qlive, M->ctx.order, s));
    SKF_TRY(d16_wgrad(M, w.mha1.qkv, W + a.x_in, d, dqkv, 3 * d, Md, s));
    SKF_TRY(d16_dgrad(M, w.mha1.qkv, dqkv, 3 * d, Md, G2, d, 1, nullptr, 0, s));
    char* t = G; G = G2; G2 = t;
  }
  M->ctx.clear_live();
  SKF_TRY(skf_embed_bwd_sorted_bf16(M->at<char>(P.emb_sort[1]), B, Ld, G, c.vocab_size, d, M->G(L.dec_emb), rate, site_dec_embed(N), M->state, s));
  SKF_TRY(ln16_reduce(M, true, s));
  if (M->bucket_ready[0] && M->n_buckets == 2) SKF_HIP(hipEventRecord(M->bucket_ready[0], s));
  // ---------------- expander, classifier (fp32), bottleneck
  SKF_TRY(skf_expander_bwd_bf16(dpre, M->at<float>(P.emb), M->P(L.exp_w), B, Le, d, demb, 0, M->G(L.exp_w), M->G(L.exp_b),
                                W + P.small_ws, P.small_ws_bytes, s));
  {
    const float* dcls = M->at<float>(P.cls_logits);
    const int splits = skf_gemm_default_splits(d, c.n_classes, B);
    SKF_TRY(skf_gemm_f32(0, 0, d, c.n_classes, B, M->at<float>(P.emb), d, dcls, c.n_classes, M->G(L.cls.w), L.cls.ld, nullptr, 0, nullptr,
                         0, 0, splits, M->G(L.cls.b), 0, W + P.slab, P.slab_bytes, SKF_PREC_F32, s));
    SKF_TRY(skf_gemm_f32(1, 1, B, d, c.n_classes, dcls, c.n_classes, M->P(L.cls.w), L.cls.ld, demb, d, nullptr, 0, nullptr, 0, 1, 1,
                         nullptr, 0, nullptr, 0, SKF_PREC_F32, s));
  }
  char* enc_out = W + P.enc[N - 1].x2;
  SKF_TRY(skf_pool_bwd_bf16(W + P.u, M->P(L.bott_v), enc_out, M->at<float>(P.pool_a), demb, B, Le, U, d, G, M->G(L.bott_v), W + P.small_ws,
                            P.small_ws_bytes, s));
  SKF_TRY(d16_wgrad(M, L.bott_w, enc_out, d, W + P.u, U, Me, s));
  SKF_TRY(d16_dgrad(M, L.bott_w, W + P.u, U, Me, G, d, 1, nullptr, 0, s));
  for (int i = N - 1; i >= 0; --i) {
    const EncLayerP& w = L.enc[i];
    const Enc16& a = P.enc[i];
    SKF_TRY(ln16_bwd(M, w.ln2, G, a.z2, a.st2, G2, dy, Me, rate, site_enc(i, 1), s));
    SKF_TRY(d16_wgrad(M, w.f2, W + a.h, F, dy, d, Me, s));
    SKF_TRY(d16_dgrad(M, w.f2, dy, d, Me, dhb, F, 0, W + a.h, F, s, hbits16(M, a.hbits)));
    SKF_TRY(d16_wgrad(M, w.f1, W + a.x1, d, dhb, F, Me, s));
    SKF_TRY(d16_dgrad(M, w.f1, dhb, F, Me, G2, d, 1, nullptr, 0, s));
    SKF_TRY(ln16_bwd(M, w.ln1, G2, a.z1, a.st1, G, dy, Me, rate, site_enc(i, 0), s));
    SKF_TRY(d16_wgrad(M, w.mha.o, W + a.o, d, dy, d, Me, s));
    SKF_TRY(d16_dgrad(M, w.mha.o, dy, d, Me, dO, d, 0, nullptr, 0, s));
    const char* qkv = W + a.qkv;
    SKF_TRY(skf_attention_bf16_bwd_ordered(qkv, 3 * d, qkv + 2 * d, 3 * d, qkv + 4 * d, 3 * d, W + a.o, d, W + a.olo, dO, d, M->at<float>(a.astats), emask, Le, 0,
                                   B, H, Le, Le, dh, dqkv, 3 * d, dqkv + 2 * d, 3 * d, dqkv + 4 * d, 3 * d, aws, P.attn_ws_bytes, nullptr, M->ctx.order, s));
    SKF_TRY(d16_wgrad(M, w.mha.qkv, W + a.x_in, d, dqkv, 3 * d, Me, s));
    SKF_TRY(d16_dgrad(M, w.mha.qkv, dqkv, 3 * d, Me, G, d, 1, nullptr, 0, s));
  }
  SKF_TRY(skf_embed_bwd_sorted_bf16(M->at<char>(P.emb_sort[0]), B, Le, G, c.vocab_size, d, M->G(L.enc_emb), rate, site_enc_embed(), M->state, s));
  SKF_TRY(ln16_reduce(M, false, s));
  if (M->bucket_ready[M->n_buckets - 1]) SKF_HIP(hipEventRecord(M->bucket_ready[M->n_buckets - 1], s));
  return SKF_OK;
}

int issue_embed_sorts16(SkfModel* M, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Plan16& P = M->p16;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1, d = c.d_model;
  SKF_TRY(skf_embed_sort(M->at<long long>(P.inp), Le, B, Le, c.vocab_size, M->G(M->lay.enc_emb), d, M->at<char>(P.emb_sort[0]), P.emb_sort_bytes, s));
  return skf_embed_sort(M->at<long long>(P.tar), Le, B, Ld, c.vocab_size, M->G(M->lay.dec_emb), d, M->at<char>(P.emb_sort[1]), P.emb_sort_bytes, s);
}

}  // namespace skf_model_detail
