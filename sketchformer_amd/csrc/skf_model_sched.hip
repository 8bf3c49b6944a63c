// The Dense helpers of the fp32 model and its two-stream scheduler (SideSched, skf_model_internal.h): weight gradients are queued per
// layer, issued as groups on a side stream (hold / issue / flush), their split-K slabs and the LayerNorm partials reduced by one
// batched launch per phase (ReduceBatch).
#include "skf_model_internal.h"

namespace skf_model_detail {

int dense_fwd(SkfModel* M, const DenseP& w, const float* x, int rows, float* y, int act, hipStream_t s) {
  return skf_gemm_f32(1, 0, rows, w.out, w.in, x, w.in, M->P(w.w), w.ld, y, w.out, M->P(w.b), act, nullptr, 0, 0, 1,
                      nullptr, 0, nullptr, 0, M->cfg.gemm_precision, s);
}
// y = Dense(a); z = x + dropout(y); out = LayerNorm(z): one launch where the fused kernel exists (the attention output projection
// at d_model = 128 in the split-arithmetic modes), else the Dense launch followed by the LayerNorm launch.
int dense_ln_fwd(SkfModel* M, const DenseP& w, const float* a, int rows, const float* x, float* z, const LnP& ln, float* out,
                 float* stats, float rate, unsigned site, hipStream_t s) {
  if (!M->no_ln_fuse && skf_gemm_ln_residual_supported(rows, w.out, w.in, M->cfg.gemm_precision)) {
    const int rc = skf_gemm_ln_residual_f32(rows, w.out, w.in, a, w.in, M->P(w.w), w.ld, M->P(w.b), x, M->P(ln.g), M->P(ln.b), z, out, stats,
                                            rate, site, M->state, M->cfg.gemm_precision, s);
    // the shape test above does not see pitches / alignment: a launch the fused entry declines takes the general pair (from now on)
    if (rc != SKF_EUNSUPPORTED) return rc;
    M->no_ln_fuse = true;
  }
  SKF_TRY(dense_fwd(M, w, a, rows, z, 0, s));
  return skf_layernorm_residual_fwd(x, z, M->P(ln.g), M->P(ln.b), out, stats, rows, w.out, rate, site, M->state, s);
}
// sign-bit buffer of an ffn hidden tensor (rows x dff from d inputs), or null when the shape has no such path
void* hbits_of(SkfModel* M, size_t off, int rows) {
  if (M->ctx.ffn_fused) return M->at<char>(off);      // (the fused block always writes / reads its own sign-bit words)
  if (M->no_relu_bits || !skf_gemm_relu_bits_bytes(rows, M->cfg.dff, M->cfg.d_model, M->cfg.gemm_precision)) return nullptr;
  return M->at<char>(off);
}
// ffn dense1 (relu): also leaves the sign bits of the hidden tensor for the backward when the shape has that path (bits != null)
int dense_fwd_relu_bits(SkfModel* M, const DenseP& w, const float* x, int rows, float* y, void* bits, hipStream_t s) {
  if (!bits) return dense_fwd(M, w, x, rows, y, 1, s);
  const int rc = skf_gemm_f32_bits(1, 0, rows, w.out, w.in, x, w.in, M->P(w.w), w.ld, y, w.out, M->P(w.b), 1, nullptr, 0, 0, 1,
                                   nullptr, 0, nullptr, 0, M->cfg.gemm_precision, nullptr, 0, bits, nullptr, s);
  if (rc != SKF_EUNSUPPORTED) return rc;
  // the weight-stationary dispatch declined (pitch / alignment): the general kernels, and the backward of this and every later
  // step reads the hidden tensor (relu_src) instead of sign bits nobody wrote - hbits_of() answers null from here on
  M->no_relu_bits = true;
  return dense_fwd(M, w, x, rows, y, 1, s);
}
// strided-input variant (x has row stride ldx)
int dense_fwd_ld(SkfModel* M, const DenseP& w, const float* x, int ldx, int rows, float* y, int ldy, int act, hipStream_t s) {
  return skf_gemm_f32(1, 0, rows, w.out, w.in, x, ldx, M->P(w.w), w.ld, y, ldy, M->P(w.b), act, nullptr, 0, 0, 1,
                      nullptr, 0, nullptr, 0, M->cfg.gemm_precision, s);
}
namespace {
int dense_wgrad_on(SkfModel* M, const DenseP& w, const float* x, int ldx, const float* dy, int lddy, int rows, hipStream_t s) {
  const int splits = skf_gemm_default_splits(w.in, w.out, rows);
  return skf_gemm_f32(0, 0, w.in, w.out, rows, x, ldx, dy, lddy, M->G(w.w), w.ld, nullptr, 0, nullptr, 0, 0, splits,
                      M->G(w.b), 0, M->at<char>(M->plan.gemm_ws), M->plan.gemm_ws_bytes, M->cfg.gemm_precision, s);
}
}  // namespace

// ------------------------------------------------------------------ SideSched (skf_model_internal.h)
int SideSched::create(bool captured) {
  SKF_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  if (captured) SKF_HIP(hipEventCreateWithFlags(&fork_event, hipEventDisableTiming));
  if (captured) SKF_HIP(hipEventCreateWithFlags(&join_event, hipEventDisableTiming));
  return SKF_OK;
}
void SideSched::destroy() {
  for (hipEvent_t e : events) (void)hipEventDestroy(e);
  for (hipEvent_t e : {fork_event, join_event}) if (e) (void)hipEventDestroy(e);
  if (side) (void)hipStreamDestroy(side);
}
hipEvent_t SideSched::take_event() {
  if (next_event == events.size()) {
    hipEvent_t e = nullptr;
    // Events that only order the library's own two streams on ONE device: a device-scope release is all the waiter needs
    // (the default system-scope fence of hipEventRecord writes caches back for host / peer visibility).  (The gradient-bucket
    // events handed to the caller keep the default.)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) return nullptr;
    events.push_back(e);
  }
  return events[next_event++];
}
// before_write / before_read: a queued or held group that touches `buf` is issued first (with the alternating gradient-buffer sets the
// rare case); then the main stream waits for the event the pending map holds for `buf`, unless it already waited for a later one
int SideSched::wait_side(SkfModel* M, bool writers, const void* buf, hipStream_t s) {
  auto touches = [&](const Queued& q) { return writers ? q.kind == 1 && q.dx == buf : q.dy == buf || q.x == buf; };
  for (const auto* qs : {&wq_held, &wq})
    for (const auto& q : *qs)
      if (touches(q)) { SKF_TRY(issue(M, s)); break; }
  auto& pending = writers ? pending_writers : pending_readers;
  auto it = pending.find(buf);
  if (it == pending.end()) return SKF_OK;
  if (it->second.seq > side_waited) {
    SKF_HIP(hipStreamWaitEvent(s, it->second.e, 0));
    side_waited = it->second.seq;
  }
  pending.erase(it);
  return SKF_OK;
}
// Issue the queued wgrads on the side stream: ONE ready event (everything queued on `s` so far is complete before they
// start) and ONE done event for the whole group; they are serialized among themselves and joined before the optimizer.
// The fused feed-forward backward is the FIRST kernel of a layer's backward, and its workgroups (147 KB of LDS, two waves per SIMD)
// cannot share a CU with a weight-gradient workgroup (66 KB, 272 registers): issued together - the previous layer's group on the side
// stream, the block on the main stream - they ran one after the other (134 + 136 us where 45 + 100 were expected, per layer).  So a
// layer's group is HELD at the end of the layer and goes out right behind the next layer's first launch: it then runs beside the
// LayerNorm / projection / attention kernels of that layer, which share CUs with it well.
int SideSched::issue_held(SkfModel* M, hipStream_t s, hipEvent_t ready_recorded) {
  if (wq_held.empty()) return SKF_OK;
  std::vector<Queued> cur;
  cur.swap(wq);
  wq.swap(wq_held);
  const int rc = issue(M, s, ready_recorded);
  wq.swap(cur);
  return rc;
}
int SideSched::hold(SkfModel* M, hipStream_t s) {
  if (!wq_held.empty()) SKF_TRY(issue(M, s));       // (never two groups held)
  wq_held.swap(wq);
  return SKF_OK;
}
// on_main: the queued group runs on the MAIN stream, in place (no events, no hop) - for the one weight gradient at the very end of
// the backward that the side stream would finish last (see run_backward)
int SideSched::issue(SkfModel* M, hipStream_t s, hipEvent_t ready_recorded, bool on_main) {
  SkfTailScope shield(nullptr);      // this function may run INSIDE a parked call (before_write): its side-stream launches must not take that event
  SKF_TRY(issue_held(M, s));                                   // the held group first, as a group of its own
  if (wq.empty()) return SKF_OK;
  std::vector<Queued> group;
  group.swap(wq);
  hipStream_t ws = on_main ? s : side;                         // the stream the group runs on
  hipEvent_t ready = nullptr, done = nullptr;
  if (!on_main) {
    ready = ready_recorded ? ready_recorded : take_event(); done = take_event();
    SKF_CHECK_ARG(ready && done, "event allocation failed");
    if (!ready_recorded) SKF_HIP(hipEventRecord(ready, s));   // (else: already the completion signal of the launch in front of this call)
    SKF_HIP(hipStreamWaitEvent(side, ready, 0));
  }
  // deferred input gradients first, with their own completion event: their reader must not wait for the weight gradients
  hipEvent_t dgrad_done = nullptr;
  for (const auto& q : group) {
    if (q.kind != 1) continue;
    const DenseP& w = q.w;
    SKF_TRY(skf_gemm_f32(1, 1, q.rows, w.in, w.out, q.dy, q.lddy, M->P(w.w), w.ld, q.dx, q.lddx, nullptr, 0, nullptr, 0,
                         q.accumulate, 1, nullptr, 0, nullptr, 0, M->cfg.gemm_precision, ws));
    if (!dgrad_done && !on_main) { dgrad_done = take_event(); SKF_CHECK_ARG(dgrad_done, "event allocation failed"); }
  }
  long dgrad_seq = 0;
  if (dgrad_done) { SKF_HIP(hipEventRecord(dgrad_done, side)); dgrad_seq = ++side_seq; }
  // the large problems of the group: partial tiles by ONE grouped launch (up to 8 problems each); every slab of the phase is
  // reduced by one launch in flush_wgrads()
  std::vector<SkfWgradProblem> probs;
  std::vector<const Queued*> prob_q;
  for (const auto& q : group) {
    const DenseP& w = q.w;
    if (q.kind != 0) continue;
    if ((double)w.in * w.out * q.rows <= 33554432.0) {
      // batch-sized problems (classifier, class buffers, SelfAttnV2 projection): one small-GEMM launch, no split-K slab
      SKF_TRY(dense_wgrad_on(M, w, q.x, q.ldx, q.dy, q.lddy, q.rows, ws));
      continue;
    }
    const int splits = skf_gemm_default_splits(w.in, w.out, q.rows);
    const size_t bytes = (skf_gemm_workspace_bytes(w.in, w.out, q.rows, splits, 1) + 255) & ~(size_t)255;
    SkfWgradProblem pr{};
    pr.A = q.x; pr.B = q.dy; pr.slab = M->red.take_slab(M, bytes, probs.size()); pr.slab_bytes = bytes;
    if (!pr.slab) return SKF_EINVAL;
    pr.row_blocks = q.blocks32; pr.row_block_rows = 32;
    pr.M = w.in; pr.N = w.out; pr.K = q.rows; pr.lda = q.ldx; pr.ldb = q.lddy; pr.splits = splits; pr.with_bias_grad = 1;
    probs.push_back(pr); prob_q.push_back(&q);
  }
  // (measured: grouping the 1-3 GFLOP problems of cfg 2 shortens the step by 0.6 %, grouping the 3-13 GFLOP ones of cfg 3 lengthens
  //  it by 1.3 % - those fill the chip for ~90 us each and gain nothing from sharing a grid)
  bool small = true;
  for (const auto& pr : probs) small = small && 2.0 * pr.M * pr.N * pr.K < 4e9;
  const size_t gmax = small ? 8 : 1;
  for (size_t b0 = 0; b0 < probs.size(); b0 += gmax) {
    const int nb = (int)std::min<size_t>(gmax, probs.size() - b0);
    SKF_TRY(skf_gemm_wgrad_partial_group(probs.data() + b0, nb, M->cfg.gemm_precision, ws));
  }
  for (size_t i = 0; i < probs.size(); ++i) {
    const DenseP& w = prob_q[i]->w;
    SkfReduceDesc d;
    d.slab = probs[i].slab; d.C = M->G(w.w); d.bias_grad = M->G(w.b); d.splits = probs[i].splits_used; d.M = w.in; d.N = w.out; d.ldc = w.ld;
    d.block_begin = M->red.blocks(); d.pad = 0;
    SKF_TRY(M->red.add(d, skf_splitk_reduce_blocks(w.in, w.out)));
  }
  M->red.side_used = true;                                         // (the slabs are reduced by the batched launch either way)
  // the single launches that leave with the group (the decoder embedding gradient) go last: in front they would push the weight
  // gradients towards the next fused feed-forward launch of the main stream (see issue_held)
  for (const auto& q : group)
    if (q.kind == 2) SKF_TRY(q.run(ws));
  if (on_main) return SKF_OK;                                  // same stream as every later reader / writer of the operands: nothing to track
  SKF_HIP(hipEventRecord(done, side));
  const long done_seq = ++side_seq;
  for (const auto& q : group) {
    pending_readers[q.dy] = SideEvent{done, done_seq};
    if (q.x) pending_readers[q.x] = SideEvent{done, done_seq};
    if (q.kind == 1) pending_writers[q.dx] = SideEvent{dgrad_done, dgrad_seq};
  }
  return SKF_OK;
}
int SideSched::join(hipStream_t s) {
  hipEvent_t e = take_event();
  SKF_CHECK_ARG(e, "event allocation failed");
  SKF_HIP(hipEventRecord(e, side));
  SKF_HIP(hipStreamWaitEvent(s, e, 0));
  pending_readers.clear();
  pending_writers.clear();
  side_waited = side_seq;        // every event recorded so far is behind the main stream
  return SKF_OK;
}
// dW = X^T dY (+ bias grad).  Two streams: queued, and issued per layer on the side stream (SideSched::issue).
int dense_wgrad(SkfModel* M, const DenseP& w, const float* x, int ldx, const float* dy, int lddy, int rows, hipStream_t s) {
  if (!M->sched.side) return dense_wgrad_on(M, w, x, ldx, dy, lddy, rows, s);
  M->sched.queue_wgrad(w, x, ldx, dy, lddy, rows, M->ctx.live_blocks(rows, 32));
  return SKF_OK;
}
// Reduce the split-K partials of the wgrads issued since the last flush (one batched launch on the side stream) and
// mark gradient bucket `bucket` complete.  final = the main stream waits for the side stream (before the optimizer).
int flush_wgrads(SkfModel* M, hipStream_t s, int bucket, bool final, bool issue_queued, bool side_behind_main) {
  if (issue_queued) SKF_TRY(M->sched.issue(M, s));      // (false: reduce what has been issued; queued / held groups stay where they are)
  const size_t begin = M->red.begin(), end = M->red.end();
  hipStream_t ready_on = s;
  bool bucket_recorded = false;
  hipStream_t side = M->sched.side;
  if (side && M->red.side_used && end > begin) {
    if (!M->red.descs_uploaded) {      // the launch sequence is fixed: descriptors are built and uploaded once (first step)
      SKF_HIP(hipMemcpy(M->at<SkfReduceDesc>(M->plan.descs) + begin, M->red.descs.data() + begin,
                        (end - begin) * sizeof(SkfReduceDesc), hipMemcpyHostToDevice));
      if (final) M->red.descs_uploaded = true;
    }
    // LayerNorm partials and the embedding gradients of this bucket were written by the main stream: the batched
    // reduction (wgrad slabs + LayerNorm partials) and the bucket-ready event are ordered after both streams
    if (final) {
      // end of the backward: the optimizer waits for this reduction anyway, so it runs on the MAIN stream behind ONE hop
      // (side -> main after the last weight gradient) instead of two (main -> side for the partials, side -> main for the result)
      SKF_TRY(M->sched.join(s));
      // the bucket-ready event rides on the reduction launch as its completion signal (skf_common.h: SKF_LAUNCH_TAIL)
      SKF_TRY(with_tail_event(M, bucket >= 0 ? M->bucket_ready[bucket] : nullptr, &bucket_recorded, [&] {
        return skf_splitk_reduce_batch(M->at<SkfReduceDesc>(M->plan.descs) + begin, (int)(end - begin), M->red.blocks(), s);
      }));
    } else {
      // (side_behind_main: the last group's ready event was recorded behind every main-stream launch of the bucket, and the side
      //  stream, in order, is behind that group: nothing to hand over)
      if (!side_behind_main) {
        hipEvent_t em = M->sched.take_event();
        SKF_CHECK_ARG(em, "event allocation failed");
        SKF_HIP(hipEventRecord(em, s));
        SKF_HIP(hipStreamWaitEvent(side, em, 0));
      }
      SKF_TRY(skf_splitk_reduce_batch(M->at<SkfReduceDesc>(M->plan.descs) + begin, (int)(end - begin), M->red.blocks(), side));
      ready_on = side;
    }
  }
  if (bucket >= 0 && M->bucket_ready[bucket] && !bucket_recorded) SKF_HIP(hipEventRecord(M->bucket_ready[bucket], ready_on));   // bucket < 0: an intermediate reduction
  M->red.end_phase(final);
  return SKF_OK;
}
int dense_dgrad(SkfModel* M, const DenseP& w, const float* dy, int lddy, int rows, float* dx, int lddx, int accumulate,
                const float* relu_src, int ld_relu, hipStream_t s, const void* relu_bits) {
  SKF_TRY(M->sched.before_write(M, dx, s));
  const int* blocks = M->ctx.live_blocks(rows, 16);
  if (relu_bits)      // relu'(hidden) from the sign bits the forward left (skf_gemm_f32_bits): the hidden tensor is not re-read
    return skf_gemm_f32_bits(1, 1, rows, w.in, w.out, dy, lddy, M->P(w.w), w.ld, dx, lddx, nullptr, 0, nullptr, 0,
                             accumulate, 1, nullptr, 0, nullptr, 0, M->cfg.gemm_precision, blocks, 16, nullptr, relu_bits, s);
  return skf_gemm_f32_rows(1, 1, rows, w.in, w.out, dy, lddy, M->P(w.w), w.ld, dx, lddx, nullptr, 0, relu_src, ld_relu,
                           accumulate, 1, nullptr, 0, nullptr, 0, M->cfg.gemm_precision, blocks, 16, s);
}

// dx (+)= dY W^T for a dx that the main stream reads much later (the encoder-output gradient sent back by the decoder's
// cross-attention K/V projections): queued behind this layer's weight gradients on the side stream; the reader calls
// before_read(dx).  Successive deferred writers of one dx stay in order (one side stream).
int dense_dgrad_deferred(SkfModel* M, const DenseP& w, const float* dy, int lddy, int rows, float* dx, int lddx, int accumulate,
                         hipStream_t s) {
  if (!M->sched.side) return dense_dgrad(M, w, dy, lddy, rows, dx, lddx, accumulate, nullptr, 0, s);
  M->sched.queue_dgrad(w, dy, lddy, rows, dx, lddx, accumulate);
  return SKF_OK;
}

// ------------------------------------------------------------------ ReduceBatch (skf_model_internal.h)
void ReduceBatch::begin_step() {
  side_used = false;
  slab_cursor = 0; desc_cursor = 0; reduce_blocks = 0; phase_desc_begin = 0; ln_cursor = 0;
}
void ReduceBatch::reset() {
  descs.clear(); descs_uploaded = false;
  slab_cursor = 0; desc_cursor = 0; ln_cursor = 0; reduce_blocks = 0; phase_desc_begin = 0;
}
int ReduceBatch::add(const SkfReduceDesc& d, int blocks) {
  // skf.h, SkfReduceDesc: the batched kernel has no scalar path - with column sums behind the tiles M*N must be a multiple of 4
  SKF_CHECK_ARG(!d.bias_grad || (((uintptr_t)d.slab & 15) == 0 && (((size_t)d.M * d.N) & 3) == 0),
                "reduce descriptor with a bias gradient: slab must be 16-byte aligned and M*N a multiple of 4");
  if (!descs_uploaded) descs.push_back(d);
  else {
    const SkfReduceDesc& o = descs[desc_cursor];
    SKF_CHECK_ARG(o.slab == d.slab && o.C == d.C && o.splits == d.splits && o.block_begin == d.block_begin, "wgrad sequence changed between steps");
  }
  reduce_blocks += blocks;
  desc_cursor += 1;
  side_used = true;
  return SKF_OK;
}
float* ReduceBatch::take_ln_partial(SkfModel* M) {
  const Plan& P = M->plan;
  if (!(ln_cursor < 5 * (size_t)M->cfg.num_layers && desc_cursor < P.n_wgrads)) {
    skf_set_error("%s: LayerNorm partial arena exhausted", __func__);
    return nullptr;
  }
  return M->at<float>(P.ln_part + ln_cursor * P.ln_part_stride);
}
float* ReduceBatch::take_slab(SkfModel* M, size_t bytes, size_t queued) {
  if (!(slab_cursor + bytes <= M->plan.slab_arena_bytes && desc_cursor + queued < M->plan.n_wgrads)) {
    skf_set_error("%s: slab arena exhausted", __func__);
    return nullptr;
  }
  float* slab = M->at<float>(M->plan.slab_arena + slab_cursor);
  slab_cursor += bytes;
  return slab;
}
void ReduceBatch::end_phase(bool final) {
  phase_desc_begin = desc_cursor;
  reduce_blocks = 0;                 // block numbering of the next batch starts again at 0
  if (final) side_used = false;
}
}  // namespace skf_model_detail
