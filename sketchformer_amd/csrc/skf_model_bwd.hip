// The fp32 backward (no autograd: the sequence is explicit) and what the train step puts on the side stream in front of it.
#include "skf_model_internal.h"

namespace skf_model_detail {
namespace {

// with_tail_event (skf_model_internal.h) with a fresh event of the step's pool, for the "main stream has reached this point" event of the weight-gradient group that
// is issued right behind `call`: *ready = the event when it rode, null when it did not (or was not wanted) - the group then records
// one of its own (SideSched::issue).
template <typename F>
int with_ready_event(SkfModel* M, bool want, hipEvent_t* ready, F call) {
  hipEvent_t e = (want && may_park(M)) ? M->sched.take_event() : nullptr;
  bool rode = false;
  const int rc = with_tail_event(M, e, &rode, call);
  *ready = rode ? e : nullptr;
  return rc;
}

int ffn_bwd(SkfModel* M, const DenseP& f1, const DenseP& f2, const float* x_in, const float* h, const float* dy,
            float* dh, float* dx_acc, int rows, hipStream_t s, const void* hbits, const void* image_t) {
  if (M->ctx.ffn_fused) {       // both input gradients in one launch; the weight gradients read dy / h and x / dh as before
    SKF_TRY(dense_wgrad(M, f2, h, f2.in, dy, f2.out, rows, s));
    SKF_TRY(M->sched.before_write(M, dh, s));
    SKF_TRY(M->sched.before_write(M, dx_acc, s));
    const int* blocks = M->ctx.live_blocks(rows, 16);
    hipEvent_t ready = nullptr;      // the held group's "main stream is here" event rides on this launch
    SKF_TRY(with_ready_event(M, M->sched.holding(), &ready, [&] {
      return skf_ffn_fused_bwd_f32(rows, M->cfg.d_model, M->cfg.dff, dy, image_t, hbits, dh, dx_acc, 1, blocks, blocks ? 16 : 0,
                                   M->cfg.gemm_precision, s);
    }));
    SKF_TRY(M->sched.issue_held(M, s, ready));
    return dense_wgrad(M, f1, x_in, f1.in, dh, f1.out, rows, s);
  }
  SKF_TRY(dense_wgrad(M, f2, h, f2.in, dy, f2.out, rows, s));
  SKF_TRY(dense_dgrad(M, f2, dy, f2.out, rows, dh, f2.in, 0, h, f2.in, s, hbits));
  SKF_TRY(dense_wgrad(M, f1, x_in, f1.in, dh, f1.out, rows, s));
  SKF_TRY(dense_dgrad(M, f1, dh, f1.out, rows, dx_acc, f1.in, 1, nullptr, 0, s));
  return SKF_OK;
}

// `splits` partial row pairs [splits][2][d] of a LayerNorm's (dgamma, dbeta) -> one descriptor of the batched split-K reduction
int ln_partials_desc(SkfModel* M, const LnP& ln, const float* part, int splits) {
  const int d = M->cfg.d_model;
  SkfReduceDesc r;
  r.slab = part; r.C = M->G(ln.g); r.bias_grad = nullptr; r.splits = splits; r.M = 1; r.N = 2 * d;
  r.ldc = 2 * d; r.block_begin = M->red.blocks(); r.pad = 0;
  SKF_TRY(M->red.add(r, skf_splitk_reduce_blocks(1, 2 * d)));
  M->red.ln_cursor += 1;
  return SKF_OK;
}

// column sums of per-sample partials part[splits][n] -> C[n] in the batched reduction (a "slab" of `splits` splits of a 1 x n matrix)
int colsum_desc(SkfModel* M, const float* part, int splits, int n, float* C) {
  SKF_CHECK_ARG(M->red.end() < M->plan.n_wgrads, "reduction descriptor table exhausted");
  SkfReduceDesc r;
  r.slab = part; r.C = C; r.bias_grad = nullptr; r.splits = splits; r.M = 1; r.N = n;
  r.ldc = n; r.block_begin = M->red.blocks(); r.pad = 0;
  return M->red.add(r, skf_splitk_reduce_blocks(1, n));
}

int ln_bwd(SkfModel* M, const LnP& ln, const float* dout, const float* z, const float* st, float* dz, float* dy,
           int rows, float rate, unsigned site, hipStream_t s) {
  const Plan& P = M->plan;
  const int d = M->cfg.d_model;
  SKF_TRY(M->sched.before_write(M, dz, s));
  if (dy != dz) SKF_TRY(M->sched.before_write(M, dy, s));
  // decoder side of a padded batch: rows behind a sample's live length have dout == 0 and are not read
  const int* ll = M->ctx.live_lengths(rows);
  const int rps = M->cfg.seq_len - 1;
  if (!M->sched.side || ln.b != ln.g + (size_t)d)
    return skf_layernorm_residual_bwd_rows(dout, z, st, M->P(ln.g), dz, dy, M->G(ln.g), M->G(ln.b), rows, d, rate,
                                           site, M->state, M->at<char>(P.small_ws), P.small_ws_bytes, ll, rps, s);
  // eager path: leave the [g][2d] partials in this LayerNorm's own slice; their column sums ride in the batched
  // split-K reduction of the wgrads (a "slab" of g splits of a 1 x 2d matrix) instead of one tiny launch per LayerNorm
  float* part = M->red.take_ln_partial(M);
  if (!part) return SKF_EINVAL;
  const size_t bytes = skf_layernorm_bwd_workspace_bytes(rows, d);
  SKF_TRY(skf_layernorm_residual_bwd_rows(dout, z, st, M->P(ln.g), dz, dy, nullptr, nullptr, rows, d, rate, site, M->state, part,
                                          bytes, ll, rps, s));
  return ln_partials_desc(M, ln, part, (int)(bytes / (8 * (size_t)d)));
}

// THE routing decision of the backward's row-owner launches: the launch takes this LayerNorm's backward and leaves its `pbytes` of
// dgamma | dbeta partials in a slice of the partial arena, to be summed by the batched reduction.  o (+ lead_w): the launch is the
// LayerNorm-backward + projection one (skf_layernorm_bwd_dgrad_lead_f32) over `rows` rows and multiplies by these Dense layers (d x d).
bool row_owner_takes_ln(const SkfModel* M, const LnP& ln, size_t pbytes, int rows = 0, const DenseP* o = nullptr, const DenseP* lead_w = nullptr) {
  const int d = M->cfg.d_model;
  auto square = [d](const DenseP* w) { return !w || (w->in == d && w->out == d); };
  return M->ctx.ffn_fused && M->sched.side && ln.b == ln.g + (size_t)d && pbytes <= M->plan.ln_part_stride && square(o) && square(lead_w) &&
         (!o || skf_layernorm_bwd_dgrad_supported(rows, d, M->cfg.gemm_precision));
}

// Both input gradients of a feed-forward block AND the backward of the LayerNorm that closes it in one launch
// (skf_ffn_fused_bwd_ln_f32), where that kernel exists and its dgamma / dbeta partials can ride in the batched reduction;
// otherwise the LayerNorm launch followed by ffn_bwd.  dout: gradient of the LayerNorm output; dx = dz + d(ffn input) is WRITTEN.
int ffn_ln_bwd(SkfModel* M, const LnP& ln, const DenseP& f1, const DenseP& f2, const float* dout, const float* z, const float* st,
               const float* x_in, const float* h, float* dy, float* dh, float* dx, int rows, float rate, unsigned site, hipStream_t s,
               const void* hbits, const void* image_t) {
  const int d = M->cfg.d_model;
  M->ctx.last_ready = nullptr;
  const size_t pbytes = (size_t)skf_ffn_fused_ln_partials(rows) * 2 * d * sizeof(float);
  if (!row_owner_takes_ln(M, ln, pbytes)) {
    SKF_TRY(ln_bwd(M, ln, dout, z, st, dx, dy, rows, rate, site, s));
    return ffn_bwd(M, f1, f2, x_in, h, dy, dh, dx, rows, s, hbits, image_t);
  }
  float* part = M->red.take_ln_partial(M);
  if (!part) return SKF_EINVAL;
  SKF_TRY(M->sched.before_write(M, dy, s));
  SKF_TRY(M->sched.before_write(M, dh, s));
  SKF_TRY(M->sched.before_write(M, dx, s));
  const int* blocks = M->ctx.live_blocks(rows, 16);
  hipEvent_t ready = nullptr;      // the held group's "main stream is here" event rides on this launch
  SKF_TRY(with_ready_event(M, M->sched.holding(), &ready, [&] {
    return skf_ffn_fused_bwd_ln_f32(rows, d, M->cfg.dff, dout, z, st, M->P(ln.g), rate, site, M->state, image_t, hbits, dy, dh, dx, part,
                                    pbytes, blocks, blocks ? 16 : 0, M->cfg.gemm_precision, s);
  }));
  SKF_TRY(ln_partials_desc(M, ln, part, skf_ffn_fused_ln_partials(rows)));
  M->ctx.last_ready = ready;                        // (nothing else reaches the main stream before this function returns: the caller may reuse it)
  SKF_TRY(M->sched.issue_held(M, s, ready));      // the previous layer's weight gradients: behind this launch (see SideSched::hold)
  SKF_TRY(dense_wgrad(M, f2, h, f2.in, dy, f2.out, rows, s));
  return dense_wgrad(M, f1, x_in, f1.in, dh, f1.out, rows, s);
}

// The backward of an attention sublayer's tail, out = LayerNorm(x + dropout(o_proj(a))): LayerNorm backward + the projection's
// input gradient in one launch (skf_layernorm_bwd_dgrad_f32) where it exists, else the two launches.  The weight gradient is queued.
// lead_a / lead_image_t (optional): the gradient of the LayerNorm output is dout + lead_a . lead_w^T, taken into the fused launch.  The
// CALLER decides that, once, with row_owner_takes_ln(.., &o, &lead_w) - where it answers false the caller's accumulating GEMM runs
// first and no lead operand is handed in (a lead operand on the two-launch branch would be dropped silently: refused).
size_t ln_oproj_partial_bytes(const SkfModel* M, int rows) { return (size_t)skf_layernorm_bwd_dgrad_partials(rows) * 2 * M->cfg.d_model * sizeof(float); }
int ln_oproj_bwd(SkfModel* M, const LnP& ln, const DenseP& o, const float* dout, const float* z, const float* st, const float* a_in,
                 float* dz, float* dy, float* da, int rows, float rate, unsigned site, hipStream_t s, const void* image_t,
                 const float* lead_a = nullptr, const void* lead_image_t = nullptr) {
  const int d = M->cfg.d_model;
  const size_t pbytes = ln_oproj_partial_bytes(M, rows);
  if (!row_owner_takes_ln(M, ln, pbytes, rows, &o)) {
    SKF_CHECK_ARG(!lead_a && !lead_image_t, "a lead operand needs the fused launch");
    SKF_TRY(ln_bwd(M, ln, dout, z, st, dz, dy, rows, rate, site, s));
    SKF_TRY(dense_wgrad(M, o, a_in, d, dy, d, rows, s));
    return dense_dgrad(M, o, dy, d, rows, da, d, 0, nullptr, 0, s);
  }
  float* part = M->red.take_ln_partial(M);
  if (!part) return SKF_EINVAL;
  SKF_TRY(M->sched.before_write(M, dz, s));
  SKF_TRY(M->sched.before_write(M, dy, s));
  SKF_TRY(M->sched.before_write(M, da, s));
  const int* blocks = M->ctx.live_blocks(rows, 16);
  SKF_TRY(skf_layernorm_bwd_dgrad_lead_f32(rows, d, dout, lead_a, lead_image_t, z, st, M->P(ln.g), rate, site, M->state, image_t, dz, dy, da, part,
                                           pbytes, blocks, blocks ? 16 : 0, M->cfg.gemm_precision, s));
  SKF_TRY(ln_partials_desc(M, ln, part, skf_layernorm_bwd_dgrad_partials(rows)));
  return dense_wgrad(M, o, a_in, d, dy, d, rows, s);
}

// Row-block lists of the decoder-side backward (token mode, split arithmetic only: the fp32-MFMA kernels ignore them)
int build_row_lists(SkfModel* M, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Plan& P = M->plan;
  M->ctx.lists_built = false;
  if (c.continuous || !do_recon(c) || c.gemm_precision == SKF_PREC_F32) return SKF_OK;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1;
  SKF_TRY(skf_target_live_len(M->at<long long>(P.tar), Le, B, Ld, M->at<int>(P.live_len), s));
  SKF_TRY(skf_row_blocks_build(M->at<int>(P.live_len), B, Ld, 16, M->at<int>(P.live16), s));
  SKF_TRY(skf_row_blocks_build(M->at<int>(P.live_len), B, Ld, 32, M->at<int>(P.live32), s));
  M->ctx.lists_built = true;
  return SKF_OK;
}

}  // namespace

int run_backward(SkfModel* M, hipStream_t s) {
  M->ctx.begin_backward();      // (the live rows are set below, for the decoder layers only)
  M->sched.begin_backward();
  M->red.begin_step();
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan& P = M->plan;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1, d = c.d_model, H = c.num_heads, dh = d / H;
  const int Me = B * Le, Md = B * Ld, N = c.num_layers;
  const float rate = c.dropout_rate;
  const long long* inp = M->at<long long>(P.inp);
  const long long* tar = M->at<long long>(P.tar);
  const unsigned char* emask = M->at<unsigned char>(P.enc_mask);
  const unsigned char* dmask = M->at<unsigned char>(P.dec_mask);
  float* G = M->at<float>(P.gA);
  float* G2 = M->at<float>(P.gB);
  float* dO = M->at<float>(P.do_);
  float* dpre = M->at<float>(P.dpre);
  float* demb = M->at<float>(P.demb);
  int layer_no = 0;     // running layer counter: picks the gradient-buffer set

  const bool bott = has_bott(c), cls = has_cls(c), recon = do_recon(c);
  float* enc_out = M->at<float>(P.enc[N - 1].x2);
  const float* pre = bott ? M->at<float>(P.pre) : enc_out;      // pre_decoder (see run_forward)
  // token mode, two streams: the decoder embedding gradient runs on the side stream (at the end of the decoder loop)
  const bool dec_emb_on_side = recon && M->sched.side && !c.continuous && P.emb_sort_bytes;
  if (recon) {
  // From the output layer to the decoder embedding every (B * Ld)-row gradient is exactly zero behind a sample's last trained position
  // (skf_row_blocks.hip): the split-arithmetic GEMMs walk the live row blocks only.  Not in continuous mode (its pen-state
  // loss has a gradient at every position), not for the fp32-MFMA kernels (they ignore the lists).
  // (the lists only depend on the staged targets: issue_embed_sorts builds them on the side stream under the forward)
  if (!M->ctx.lists_built) SKF_TRY(build_row_lists(M, s));
  if (M->ctx.lists_built) M->ctx.set_live(Md, M->at<int>(P.live_len), 16, M->at<int>(P.live16), 32, M->at<int>(P.live32));
  M->ctx.lists_built = false;
  // output layer: logits buffer now holds dlogits
  const float* dlog = M->at<float>(P.logits);
  SKF_TRY(dense_wgrad(M, L.out, M->at<float>(P.dec[N - 1].out3), d, dlog, L.out.out, Md, s));
  {
    hipEvent_t ready = nullptr;      // the group's "main stream is here" event rides on the input-gradient launch (the last of its chain)
    SKF_TRY(with_ready_event(M, true, &ready, [&] { return dense_dgrad(M, L.out, dlog, L.out.out, Md, G, d, 0, nullptr, 0, s); }));
    SKF_TRY(M->sched.issue(M, s, ready));
  }
  const unsigned char* cross_mask = c.blind_decoder_mask ? nullptr : emask;
  for (int i = N - 1; i >= 0; --i, ++layer_no) {
    const DecLayerP& w = L.dec[i];
    const DecAct& a = P.dec[i];
    const Plan::GradSet& gs = P.gs[layer_no % P.n_gs];
    float* dy3 = M->at<float>(gs.dy[0]); float* dy2 = M->at<float>(gs.dy[1]); float* dy1 = M->at<float>(gs.dy[2]);
    float* dqkv = M->at<float>(gs.dqkv); float* dkv2 = M->at<float>(gs.dkv2); float* dq2 = M->at<float>(gs.dq2);
    // out3 = LN3(out2 + drop(ffn(out2)))
    SKF_TRY(ffn_ln_bwd(M, w.ln3, w.f1, w.f2, G, M->at<float>(a.z3), M->at<float>(a.st3), M->at<float>(a.out2), M->at<float>(a.h), dy3,
                       M->at<float>(gs.dh), G2, Md, rate, site_dec(N, i, 2), s, hbits_of(M, a.hbits, Md), M->at<char>(a.img[1])));
    // out2 = LN2(out1 + drop(mha2(pre, pre, out1)))
    SKF_TRY(ln_oproj_bwd(M, w.ln2, w.mha2.o, G2, M->at<float>(a.z2), M->at<float>(a.st2), M->at<float>(a.o2), G, dy2, dO, Md, rate,
                         site_dec(N, i, 1), s, M->at<char>(a.img_o2)));
    const float* kv2 = M->at<float>(a.kv2);
    SKF_TRY(M->sched.before_write(M, dq2, s));
    SKF_TRY(M->sched.before_write(M, dkv2, s));
    const int* qlive = M->ctx.live_lengths(Md);      // decoder query rows behind it have dO == 0
    SKF_TRY(skf_attention_bwd_ordered(M->at<float>(a.q2), d, kv2, 2 * d, kv2 + d, 2 * d, M->at<float>(a.o2), d, dO, d,
                                      M->at<float>(a.astats2), cross_mask, Le, 0, B, H, Ld, Le, dh, dq2, d, dkv2, 2 * d,
                                      dkv2 + d, 2 * d, M->cfg.gemm_precision, qlive, M->ctx.order, s));
    SKF_TRY(dense_wgrad(M, w.mha2.q, M->at<float>(a.out1), d, dq2, d, Md, s));
    // d(out1) += dq2 . Wq^T: inside the LayerNorm-backward launch of the self-attention sublayer below where that kernel takes it
    const bool lead = row_owner_takes_ln(M, w.ln1, ln_oproj_partial_bytes(M, Md), Md, &w.mha1.o, &w.mha2.q);
    if (!lead) SKF_TRY(dense_dgrad(M, w.mha2.q, dq2, d, Md, G, d, 1, nullptr, 0, s));
    SKF_TRY(dense_wgrad(M, w.mha2.kv, pre, L.E, dkv2, 2 * d, Me, s));
    // (the last layer of the loop runs it on the main stream.  A deferred input gradient leaves with its layer's whole group at the end
    //  of the layer, and for this layer the reader - the expander backward - follows that point too soon to gain anything.  That is a
    //  limit of the group mechanism, not of the data: dkv2 is ready as soon as the cross-attention backward above ends.  Letting it
    //  leave right there - with the five weight gradients queued so far as a group of its own, its ready event riding on the
    //  cross-attention backward - was built and measured: the 45-us launch left the main stream and the step got 0.012 ms LONGER
    //  (5 of 6 interleaved rounds): that group then runs beside this layer's self-attention backward and the next fused feed-forward
    //  launches, which slow down by more than the move saved.  Taken out again; profiles/side_stream_moves_ab.txt)
    if (i == 0) {
      SKF_TRY(M->sched.before_read(M, dpre, s));   // the side-stream writers of the layers above have finished accumulating
      SKF_TRY(dense_dgrad(M, w.mha2.kv, dkv2, 2 * d, Me, dpre, L.E, i != N - 1, nullptr, 0, s));
    } else SKF_TRY(dense_dgrad_deferred(M, w.mha2.kv, dkv2, 2 * d, Me, dpre, L.E, i != N - 1, s));
    // out1 = LN1(x + drop(mha1(x,x,x)))
    SKF_TRY(ln_oproj_bwd(M, w.ln1, w.mha1.o, G, M->at<float>(a.z1), M->at<float>(a.st1), M->at<float>(a.o1), G2, dy1, dO, Md, rate,
                         site_dec(N, i, 0), s, M->at<char>(a.img_o1), lead ? dq2 : nullptr, lead ? M->at<char>(a.img_q2t) : nullptr));
    const float* qkv = M->at<float>(a.qkv);
    SKF_TRY(M->sched.before_write(M, dqkv, s));
    SKF_TRY(skf_attention_bwd_ordered(qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, M->at<float>(a.o1), d, dO, d,
                                      M->at<float>(a.astats1), dmask, Ld, 1, B, H, Ld, Ld, dh, dqkv, 3 * d, dqkv + d, 3 * d,
                                      dqkv + 2 * d, 3 * d, M->cfg.gemm_precision, qlive, M->ctx.order, s));
    SKF_TRY(dense_wgrad(M, w.mha1.qkv, M->at<float>(a.x_in), d, dqkv, 3 * d, Md, s));
    // the 8 weight gradients of this layer: one event pair - held until the next layer's fused feed-forward launch is queued
    const bool hold = M->ctx.ffn_fused && i > 0;
    hipEvent_t ready = nullptr;      // not held: the group's event rides on this layer's last launch
    SKF_TRY(with_ready_event(M, !hold, &ready, [&] { return dense_dgrad(M, w.mha1.qkv, dqkv, 3 * d, Md, G2, d, 1, nullptr, 0, s); }));
    float* t = G; G = G2; G2 = t;
    // Token mode, two streams: the decoder embedding gradient reads G, the input gradient that the launch above has just written, and
    // only the bucket's reduction - side stream - consumes its result.  It leaves with layer 0's group, as its last launch (behind the
    // ready event that rides on the launch above), and the group registers G as read by the side stream (before_write) - the
    // encoder-side backward below keeps out of that buffer.
    if (i == 0 && dec_emb_on_side) {
      const float* dx0 = G;
      char* sorted = M->at<char>(P.emb_sort[1]);
      float* dtable = M->G(L.dec_emb);
      const int V = c.vocab_size;
      M->sched.queue_launch(dx0, [M, sorted, dtable, dx0, B, Ld, V, d, rate, N](hipStream_t on) {
        return skf_embed_bwd_sorted(sorted, B, Ld, dx0, V, d, dtable, rate, site_dec_embed(N), M->state, on);
      });
    }
    if (hold) SKF_TRY(M->sched.hold(M, s));
    else SKF_TRY(M->sched.issue(M, s, ready));
  }
  M->ctx.clear_live();
  // The step metrics, left here by run_forward: nothing on the device reads M->metrics during the step, so the launch goes to the side
  // stream.  It reads the token loss sums (main stream) and the class loss sums (side stream, in front of the K|V projections): the
  // side stream has waited for the ready event of layer 0's group, recorded behind the whole decoder backward and so behind the token
  // cross-entropy, and is in order behind its own class cross-entropy - no event of its own.  Here and not behind the output layer's
  // group, which would do for the order: from there to this point the side stream is busy without a break, and whatever is put in
  // front pushes every layer's weight gradients towards the next fused feed-forward launch (profiles/side_stream_moves_ab.txt).
  // The step's final join (flush_wgrads) puts the main stream behind this launch: the step still ends with the metrics complete, and
  // the next step's loss launches - the token loss on the main stream behind that join, the class loss on the in-order side stream -
  // cannot overtake this read of the four sums, however many steps the host queues without synchronising.
  if (M->ctx.metrics_deferred) {
    M->ctx.metrics_deferred = false;
    SKF_TRY(metrics_update(M, M->sched.side));
  }
  // decoder embedding (the continuous form and the unsorted one stay on the main stream: they use small_ws / a memset)
  if (c.continuous) {
    SKF_TRY(skf_embed_continuous_bwd(M->at<float>(P.tar), Le, B, Ld, G, d, M->G(L.dec_embd.w), M->G(L.dec_embd.b), rate,
                                     site_dec_embed(N), M->state, M->at<char>(P.small_ws), P.small_ws_bytes, s));
  } else if (dec_emb_on_side) {
    // (issued with layer 0's group above)
  } else if (P.emb_sort_bytes) {
    SKF_TRY(skf_embed_bwd_sorted(M->at<char>(P.emb_sort[1]), B, Ld, G, c.vocab_size, d, M->G(L.dec_emb), rate, site_dec_embed(N), M->state, s));
  } else {
    SKF_HIP(hipMemsetAsync(M->G(L.dec_emb), 0, (size_t)c.vocab_size * d * sizeof(float), s));
    SKF_TRY(skf_embed_bwd(tar, Le, B, Ld, G, c.vocab_size, d, M->G(L.dec_emb), rate, site_dec_embed(N), M->state, s));
  }
  // every gradient of [decoder embedding .. output layer] is issued: first bucket of the flat buffer.  With the embedding gradient on
  // the side stream, the reduction and bucket_ready[0] follow it and layer 0's group on that in-order stream, and the group's ready
  // event was recorded behind every main-stream launch of the bucket (the LayerNorm partials): no hand-over.
  if (M->n_buckets == 2) SKF_TRY(flush_wgrads(M, s, 0, false, true, dec_emb_on_side));
  SKF_TRY(M->sched.before_read(M, dpre, s));     // the deferred K/V-projection input gradients (side stream) are complete
  }   // recon
  const int E = L.E, Ua = L.Ua, U = c.lowerdim, NB = c.class_buffer_layers;
  hipEvent_t bott_ready = nullptr;
  if (bott) {
    // expander, classifier
    const bool defer_sums = M->sched.side && Ua <= 4096;      // (wherever the batched reduction runs: the eager step and its two-stream capture)
    float* xp1 = M->at<float>(P.bott_part);
    float* xp2 = xp1 + (size_t)B * Le;
    float* pvp = xp2 + (size_t)B * Le;
    if (recon && defer_sums) {
      SKF_TRY(skf_expander_bwd_partials(dpre, M->at<float>(P.emb), M->P(L.exp_w), B, Le, E, demb, 0, xp1, xp2, s));
      SKF_TRY(colsum_desc(M, xp1, B, Le, M->G(L.exp_w)));
      SKF_TRY(colsum_desc(M, xp2, B, Le, M->G(L.exp_b)));
    } else if (recon)
      SKF_TRY(skf_expander_bwd(dpre, M->at<float>(P.emb), M->P(L.exp_w), B, Le, E, demb, 0, M->G(L.exp_w), M->G(L.exp_b),
                               M->at<char>(P.small_ws), P.small_ws_bytes, s));
    const int acc_emb = recon ? 1 : 0;        // without a decoder the class head is the only source of d(embedding)
    // classifier (+ class buffers): d fc_i = dropout'(.) then relu'(.) - both are element-wise masks and commute
    const float* dcls = M->at<float>(P.cls_logits);
    if (cls && NB == 0) {
      SKF_TRY(dense_wgrad(M, L.cls, M->at<float>(P.emb), E, dcls, c.n_classes, B, s));
      SKF_TRY(dense_dgrad(M, L.cls, dcls, c.n_classes, B, demb, E, acc_emb, nullptr, 0, s));
    } else if (cls) {
      float* dz = M->at<float>(P.dcb[0]);
      float* dz2 = M->at<float>(P.dcb[1]);
      SKF_TRY(M->sched.before_write(M, dz, s));
      SKF_TRY(dense_wgrad(M, L.cls, M->at<float>(P.cb_f[NB - 1]), U, dcls, c.n_classes, B, s));
      SKF_TRY(dense_dgrad(M, L.cls, dcls, c.n_classes, B, dz, U, 0, M->at<float>(P.cb_h[NB - 1]), U, s));
      for (int i = NB - 1; i >= 0; --i) {
        SKF_TRY(skf_dropout(dz, dz, (size_t)B * U, c.class_dropout, site_class(N, i), M->state, s));
        const float* in = i == 0 ? M->at<float>(P.emb) : M->at<float>(P.cb_f[i - 1]);
        const int in_w = i == 0 ? E : U;
        SKF_TRY(dense_wgrad(M, L.cbuf[i], in, in_w, dz, U, B, s));
        if (i == 0) {
          SKF_TRY(dense_dgrad(M, L.cbuf[0], dz, U, B, demb, E, acc_emb, nullptr, 0, s));
        } else {
          SKF_TRY(M->sched.before_write(M, dz2, s));
          SKF_TRY(dense_dgrad(M, L.cbuf[i], dz, U, B, dz2, U, 0, M->at<float>(P.cb_h[i - 1]), U, s));
          float* t = dz; dz = dz2; dz2 = t;
        }
      }
    }
    // bottleneck
    const float* dpool = demb;
    if (c.attn_version == 2) {
      SKF_TRY(M->sched.before_write(M, M->at<float>(P.dpooled), s));
      SKF_TRY(dense_wgrad(M, L.bott_e, M->at<float>(P.pooled), d, demb, U, B, s));
      SKF_TRY(dense_dgrad(M, L.bott_e, demb, U, B, M->at<float>(P.dpooled), d, 0, nullptr, 0, s));
      dpool = M->at<float>(P.dpooled);
    }
    // The side stream's decoder embedding gradient reads G behind layer 0's weight gradients, long after the main stream is here
    // (even as the FIRST launch of that group it held the pooling backward up for 16 us: profiles/side_stream_moves_ab.txt).  So the
    // encoder-side gradient alternates between G2 - free, its last reader was layer 0's self-attention LayerNorm backward on this
    // stream - and the plan's third buffer, and the main stream never waits for that read.
    if (dec_emb_on_side) { G = G2; G2 = M->at<float>(P.gC); }
    SKF_TRY(M->sched.before_write(M, G, s));
    if (defer_sums) {
      SKF_TRY(skf_pool_bwd_partials(M->at<float>(P.u), M->P(L.bott_v), enc_out, M->at<float>(P.pool_a), dpool, B, Le, Ua, d, G, pvp, s));
      SKF_TRY(colsum_desc(M, pvp, B, Ua, M->G(L.bott_v)));
    } else
    SKF_TRY(skf_pool_bwd(M->at<float>(P.u), M->P(L.bott_v), enc_out, M->at<float>(P.pool_a), dpool, B, Le, Ua, d,
                         G, M->G(L.bott_v), M->at<char>(P.small_ws), P.small_ws_bytes, s));
    SKF_TRY(dense_wgrad(M, L.bott_w, enc_out, d, M->at<float>(P.u), Ua, Me, s));
    SKF_TRY(with_ready_event(M, true, &bott_ready, [&] { return dense_dgrad(M, L.bott_w, M->at<float>(P.u), Ua, Me, G, d, 1, nullptr, 0, s); }));
  } else {
    // no bottleneck: d(enc_output) is what the cross-attention K/V projections of all decoder layers sent back
    float* spare = (G == M->at<float>(P.gA)) ? M->at<float>(P.gB) : M->at<float>(P.gA);
    G = dpre; G2 = spare;
  }
  SKF_TRY(M->sched.issue(M, s, bott_ready));            // expander / classifier / bottleneck group
  for (int i = N - 1; i >= 0; --i, ++layer_no) {
    const EncLayerP& w = L.enc[i];
    const EncAct& a = P.enc[i];
    const Plan::GradSet& gs = P.gs[layer_no % P.n_gs];
    float* dy2 = M->at<float>(gs.dy[0]); float* dy1 = M->at<float>(gs.dy[1]);
    float* dqkv = M->at<float>(gs.dqkv);
    SKF_TRY(ffn_ln_bwd(M, w.ln2, w.f1, w.f2, G, M->at<float>(a.z2), M->at<float>(a.st2), M->at<float>(a.x1), M->at<float>(a.h), dy2,
                       M->at<float>(gs.dh), G2, Me, rate, site_enc(i, 1), s, hbits_of(M, a.hbits, Me), M->at<char>(a.img[1])));
    // last layer of the backward: nothing is left on the main stream to hide a whole layer's weight gradients behind
    // (only the embedding gradient follows), so they go out per sublayer - the step's tail before Adam is one wgrad, not four
    // (the fused launch's completion signal already served the held group as its "main stream is here" event: this group shares it)
    if (i == 0) SKF_TRY(M->sched.issue(M, s, M->ctx.last_ready));
    M->ctx.last_ready = nullptr;
    {
      hipEvent_t ready = nullptr;
      SKF_TRY(with_ready_event(M, i == 0, &ready, [&] {
        return ln_oproj_bwd(M, w.ln1, w.mha.o, G2, M->at<float>(a.z1), M->at<float>(a.st1), M->at<float>(a.o), G, dy1, dO, Me, rate,
                            site_enc(i, 0), s, M->at<char>(a.img_o));
      }));
      if (i == 0) SKF_TRY(M->sched.issue(M, s, ready));
    }
    const float* qkv = M->at<float>(a.qkv);
    SKF_TRY(M->sched.before_write(M, dqkv, s));
    SKF_TRY(skf_attention_bwd_ordered(qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, M->at<float>(a.o), d, dO, d,
                                      M->at<float>(a.astats), emask, Le, 0, B, H, Le, Le, dh, dqkv, 3 * d, dqkv + d, 3 * d,
                                      dqkv + 2 * d, 3 * d, M->cfg.gemm_precision, nullptr, M->ctx.order, s));
    SKF_TRY(dense_wgrad(M, w.mha.qkv, M->at<float>(a.x_in), d, dqkv, 3 * d, Me, s));
    // last layer of the backward: the weight gradient only needs dqkv, so it goes out BEFORE the input-gradient GEMM - the hop
    // to the side stream and the kernel itself then run under that GEMM and the embedding gradient instead of behind them.
    // Round 6: it runs on the MAIN stream.  The side stream still has this layer's feed-forward and output-projection gradients
    // queued behind the held group of the layer above and finished ~20 us AFTER the main stream's last kernel
    // (profiles/r06h_timeline.txt: 34 us of idle main stream in front of the final reduction); with the 18-us q|k|v gradient in line
    // here both streams end together and the final reduction starts without waiting for a hop.
    if (i == 0) SKF_TRY(M->sched.issue(M, s, nullptr, !M->sched.holding()));
    SKF_TRY(dense_dgrad(M, w.mha.qkv, dqkv, 3 * d, Me, G, d, 1, nullptr, 0, s));
    if (M->ctx.ffn_fused && i > 0) SKF_TRY(M->sched.hold(M, s));
    else SKF_TRY(M->sched.issue(M, s));
    // half-way through the encoder: the slabs and LayerNorm partials finished so far are reduced on the side stream now, under the
    // remaining layers - the final reduction, which the optimizer waits for on the main stream, shrinks to the last layers' share
    // (with a held group: only what is already on the side stream - issuing the held group here would put it beside the next layer's
    //  fused feed-forward launch again)
    // (not with the fused feed-forward blocks: the reduction launch lands beside a fused launch it cannot share CUs with - A/B 3.95 vs 3.99 ms)
    if (!M->ctx.ffn_fused && M->sched.side && N >= 2 && i == N / 2) SKF_TRY(flush_wgrads(M, s, -1, false, !M->sched.holding()));
  }
  if (c.continuous) {
    SKF_TRY(skf_embed_continuous_bwd(M->at<float>(P.inp), Le, B, Le, G, d, M->G(L.enc_embd.w), M->G(L.enc_embd.b), rate,
                                     site_enc_embed(), M->state, M->at<char>(P.small_ws), P.small_ws_bytes, s));
  } else {
    if (P.emb_sort_bytes) {
      SKF_TRY(skf_embed_bwd_sorted(M->at<char>(P.emb_sort[0]), B, Le, G, c.vocab_size, d, M->G(L.enc_emb), rate, site_enc_embed(),
                                   M->state, s));
    } else {
      SKF_HIP(hipMemsetAsync(M->G(L.enc_emb), 0, (size_t)c.vocab_size * d * sizeof(float), s));
      SKF_TRY(skf_embed_bwd(inp, Le, B, Le, G, c.vocab_size, d, M->G(L.enc_emb), rate, site_enc_embed(), M->state, s));
    }
  }
  return flush_wgrads(M, s, M->n_buckets - 1, true);
}

// The embedding gradients' counting sorts depend on the staged tokens only.  Eager path with a decoder: side stream, under
// the forward (the main stream joins the side stream at the first cross-attention, long before the backward reads the
// sorted positions); otherwise (hipGraph capture, encoder-only configurations) in place on the main stream.
int issue_embed_sorts(SkfModel* M, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  const Layout& L = M->lay;
  const Plan& P = M->plan;
  if (!P.emb_sort_bytes) return SKF_OK;
  const int B = c.batch, Le = c.seq_len, Ld = c.seq_len - 1, d = c.d_model;
  hipStream_t ss = s;
  if (M->sched.side && do_recon(c)) {
    // (the staged inputs are all the side stream's first launches read: it waits for the staging launch's own completion signal,
    //  no packet of its own on the main stream)
    hipEvent_t staged = (M->inputs_staged && M->inputs_staged_valid && !g_capturing) ? M->inputs_staged : nullptr;
    if (!staged) {
      staged = M->sched.take_event();
      SKF_CHECK_ARG(staged, "event allocation failed");
      SKF_HIP(hipEventRecord(staged, s));
    }
    SKF_HIP(hipStreamWaitEvent(M->sched.side, staged, 0));
    ss = M->sched.side;
    // first on the side stream: what the forward does not need before its first attention (forward_preamble) - the main stream goes
    // straight to the embedding and the first q|k|v projection (30 us of one-workgroup and short launches off the critical path)
    hipEvent_t masks = M->sched.take_event(), ready = M->sched.take_event();
    SKF_CHECK_ARG(masks && ready, "event allocation failed");
    SKF_TRY(forward_preamble(M, true, false, ss, masks));
    SKF_HIP(hipEventRecord(ready, ss));
    M->ctx.masks_ready = masks; M->ctx.pre_ready = ready;
  }
  SKF_TRY(skf_embed_sort(M->at<long long>(P.inp), Le, B, Le, c.vocab_size, M->G(L.enc_emb), d, M->at<char>(P.emb_sort[0]),
                         P.emb_sort_bytes, ss));
  if (do_recon(c))
    SKF_TRY(skf_embed_sort(M->at<long long>(P.tar), Le, B, Ld, c.vocab_size, M->G(L.dec_emb), d, M->at<char>(P.emb_sort[1]),
                           P.emb_sort_bytes, ss));
  return build_row_lists(M, ss);
}
}  // namespace skf_model_detail
