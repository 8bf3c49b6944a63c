// KV-cached greedy reconstruction (models/sketchformer.py:255-311).  The reference re-runs the decoder on the whole
// prefix for every token; one step here touches only the newest position (rows = batch):
//   x = embed(token_i) * sqrt(d) + pos[i]                                   (transformer.py:325-334, dropout off)
//   per layer: q = x Wq ; [k|v] = x [Wk|Wv] written straight into cache row i ; attention over keys 0..i with the
//   target padding mask (look-ahead is implicit: later keys do not exist yet) ; LN ; cross attention over the
//   cached K/V of pre_decoder ; LN ; FFN ; LN                               (transformer.py:245-262)
//   logits of position i -> argmax / stroke-5 row -> appended                (sketchformer.py:285-301)
// The request (DecodeRequest, skf_model_internal.h).  attn (optional): the softmax rows of every position, (2N, B, H, max_steps, Le) - see skf_model_greedy_decode_attn.
// smp (optional, token mode, checked by the caller): the tokens are drawn (skf_model_sample_decode) with the streams stream_ids_host
// (B ints, null = 0 .. B-1); only the selection differs, and the layer-by-layer steps are then issued eagerly.
//
// bm (optional, token mode, checked by the caller): beam search (skf_model_beam_decode).  The batch holds n = B / W sketches, the
// embedding and expected_len_host have n rows and are replicated into the W rows of a sketch on the device; a position is the beam
// instantiation of the one-launch kernel plus beam_advance_kernel (always: there are no beams on the layer-by-layer path), and the
// hypotheses are gathered through the last ancestry table into bm_out.
//
// pfx (optional, token mode, the one-launch kernel only; checked by the caller): sketch completion (skf_model_prefix_decode,
// skf_model_beam_prefix_decode; the rule is in include/skf.h).  The prefix and its lengths go to areas of the plan (replicated like the
// embedding under beam search), the position kernel forces them, and unless pfx->stepwise (or beams) asks for one position launch per
// forced position, skf_decode_prefill_launch produces their cache rows first and the position loop starts at the shortest prefix.
//
// A bf16-trained model decodes the same way, in fp32 on the MASTER weights (only the embedding it starts from comes from the bf16
// encoder), and only through the one-launch-per-position kernel.  What differs between the two plans is in the view below.
#include "skf_model_internal.h"

namespace skf_model_detail {
namespace {

struct DecodeView {
  const DecodeAreas* areas = nullptr;
  float* emb = nullptr;             // (B, E) bottleneck embedding the expander reads; null without a bottleneck
  float* pre = nullptr;             // (B, L, E) pre_decoder: written by the expander, or a copy of the caller's (B, L, d) encoder output
  float* enc_out = nullptr;         // no bottleneck: pre_decoder when the caller passes no embedding of its own
  std::vector<float*> kv2, cache;   // per layer: cross K|V of pre_decoder, self K|V of the positions so far
  int kv2_precision = 0;            // arithmetic of the cross K|V projection
  bool classify = false;            // also run the class head on the embedding (classify_from_embedding)
  bool layerwise = false;           // the plan has the layer-by-layer step's buffers; else the one-launch kernel or nothing
};

DecodeView decode_view(SkfModel* M) {
  const SkfConfig& c = M->cfg;
  const int N = c.num_layers;
  DecodeView V;
  V.areas = M->bf16 ? &M->p16.dca : &M->plan.dca;
  for (int l = 0; l < N; ++l) V.cache.push_back(M->at<float>(V.areas->cache[l]));
  if (M->bf16) {        // (skf_config_validate: a bf16 model has a bottleneck of width d)
    V.emb = M->at<float>(M->p16.emb); V.pre = M->at<float>(V.areas->pre);
    for (int l = 0; l < N; ++l) V.kv2.push_back(M->at<float>(V.areas->kv2[l]));
    V.kv2_precision = SKF_PREC_BF16X6;
    return V;
  }
  const Plan& P = M->plan;
  V.emb = has_bott(c) ? M->at<float>(P.emb) : nullptr;
  V.pre = M->at<float>(P.pre); V.enc_out = M->at<float>(P.enc[N - 1].x2);
  for (int l = 0; l < N; ++l) V.kv2.push_back(M->at<float>(P.dec[l].kv2));
  V.kv2_precision = c.gemm_precision;
  V.classify = has_cls(c);
  V.layerwise = true;
  return V;
}

// One run_decode call: the request, the dimensions, and what its pieces share - where the running output and the per-call scalars
// live, the optional beam / sampling state, the parameters of the one-launch kernel.  The pieces run once each, in the order below.
struct DecodeRun {
  SkfModel* const M;
  const DecodeRequest& rq;
  hipStream_t const s;
  const SkfConfig& c;
  const Layout& L;
  const Plan& P;                             // (the layer-by-layer step and the class head: fp32 plan only)
  const DecodeView V;
  const DecodeAreas& A;
  const int B, Le, d, H, dh, N, F;
  const int T;                               // columns of the output buffer
  const int Vout;
  const int W, nsk;                          // beam search: nsk sketches in rows g W + k
  const int Ti;                              // the running output lives in an internal (B, Le+1) image so that the captured step has constant arguments
  const size_t aw_blk;                       // one (B, H, max_steps, Le) block of the attention weights
  const float* pre = nullptr;                // pre_decoder
  int *eos_seen = nullptr, *done_step = nullptr, *step_dev = nullptr;
  long long* dyn = nullptr;
  unsigned char* selfmask = nullptr;
  long long* tokens = nullptr;
  float* cont = nullptr;
  int* limit = nullptr;                      // per-sample key limit of the cross attention (non-blind only)
  SkfBeamState bs{};
  int* stream_ids = nullptr;
  long long* pfx_tok = nullptr;              // (B, Le) the prefix on the device
  int* pfx_len = nullptr;
  int pfx_min = 0, pfx_max = 0;              // the shortest and the longest prefix of the B rows
  bool prefill = false;
  bool fused = false, use_graph = false;
  SkfDecodeFused fp{};

  DecodeRun(SkfModel* model, const DecodeRequest& request, hipStream_t stream)
      : M(model), rq(request), s(stream), c(model->cfg), L(model->lay), P(model->plan), V(decode_view(model)), A(*V.areas),
        B(c.batch), Le(c.seq_len), d(c.d_model), H(c.num_heads), dh(d / H), N(c.num_layers), F(c.dff), T(request.max_steps + 1),
        Vout(c.continuous ? 5 : c.vocab_size), W(request.bm ? request.bm->beam_width : 1), nsk(B / W), Ti(Le + 1),
        aw_blk((size_t)B * H * request.max_steps * Le) {}
  int decode_setup();          // embedding, limits, beam state, stream ids; expander, cross K|V, class head
  int fill_fused_params();     // which step runs; the one-launch kernel's parameters
  int issue_step();            // one position, layer by layer ...
  int capture_step();          // ... captured once into M->g_dec
  int issue_position();
  int decode_positions();      // the position loop and the hand-over of the columns
};

int DecodeRun::decode_setup() {
  // the embedding is (B, E) with a bottleneck, else the whole encoder output (B, L, d) = pre_decoder itself
  pre = V.pre;
  if (rq.bm) {                                              // (n, ...) rows, each replicated into its sketch's W rows
    SKF_TRY(skf_beam_replicate(V.emb ? V.emb : V.pre, rq.embedding, nsk, W, V.emb ? (size_t)L.E : (size_t)Le * d, s));
  } else if (V.emb) {
    if (rq.embedding && rq.embedding != V.emb)
      SKF_HIP(hipMemcpyAsync(V.emb, rq.embedding, (size_t)B * L.E * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else if (rq.embedding && rq.embedding != V.enc_out) {
    SKF_HIP(hipMemcpyAsync(V.pre, rq.embedding, (size_t)B * Le * d * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    pre = V.enc_out;
  }
  eos_seen = M->at<int>(A.flags);
  done_step = eos_seen + B;
  dyn = M->at<long long>(A.dyn);             // [0] n_valid, [1] eos  (read by the selection kernel)
  step_dev = reinterpret_cast<int*>(dyn + 4);      // index of the position being decoded
  selfmask = M->at<unsigned char>(A.mask);
  tokens = c.continuous ? nullptr : M->at<long long>(A.img);
  cont = c.continuous ? M->at<float>(A.img) : nullptr;
  SKF_TRY(skf_decode_init(tokens, Ti, cont, Ti, selfmask, Le + 1, eos_seen, done_step, B, rq.sos, step_dev, s));
  M->dec_dyn_host[0] = rq.n_valid; M->dec_dyn_host[1] = rq.eos;
  SKF_HIP(hipMemcpyAsync(dyn, M->dec_dyn_host, 2 * sizeof(long long), hipMemcpyHostToDevice, s));
  if (!c.blind_decoder_mask) {
    limit = M->at<int>(A.limit);
    if (rq.bm) {                                            // one limit per sketch, through the area's second half
      SKF_HIP(hipMemcpyAsync(limit + B, rq.expected_len_host, (size_t)nsk * sizeof(int), hipMemcpyHostToDevice, s));
      SKF_TRY(skf_beam_replicate(limit, limit + B, nsk, W, 1, s));
    } else if (rq.expected_len_host) SKF_HIP(hipMemcpyAsync(limit, rq.expected_len_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    else SKF_HIP(hipMemsetAsync(limit, 0xff, (size_t)B * sizeof(int), s));        // -1: nattn = step + 1
  }
  if (rq.bm) {
    bs.n = nsk; bs.W = W; bs.B = B;
    bs.cand_lp = M->at<float>(A.cand); bs.cand_tok = reinterpret_cast<int*>(bs.cand_lp + (size_t)B * SKF_BEAM_MAX);
    bs.scores = M->at<float>(A.beam); bs.finished = reinterpret_cast<int*>(bs.scores + B); bs.lengths = bs.finished + B;
    bs.anc = M->at<int>(A.anc); bs.anc_ld = Le + 1;
    bs.tokens = tokens; bs.Ti = Ti; bs.selfmask = selfmask; bs.mask_ld = Le + 1;
    bs.done_step = done_step; bs.step_dev = step_dev; bs.ticket = done_step + 1; bs.dyn = dyn;
    SKF_TRY(skf_beam_init(bs, s));
  }
  if (rq.smp) {
    stream_ids = M->at<int>(A.limit) + B;
    M->dec_stream_host.resize(B);
    for (int b = 0; b < B; ++b) M->dec_stream_host[b] = rq.stream_ids_host ? rq.stream_ids_host[b] : b;
    SKF_HIP(hipMemcpyAsync(stream_ids, M->dec_stream_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
  }
  if (rq.pfx) {
    const int rows = rq.bm ? nsk : B;
    pfx_tok = M->at<long long>(A.pfx_tok); pfx_len = M->at<int>(A.pfx_len);
    M->dec_pfx_len_host.assign(rq.pfx->len_host, rq.pfx->len_host + rows);
    pfx_min = pfx_max = M->dec_pfx_len_host[0];
    for (int v : M->dec_pfx_len_host) { pfx_min = v < pfx_min ? v : pfx_min; pfx_max = v > pfx_max ? v : pfx_max; }
    if (pfx_max > 0)
      SKF_HIP(hipMemcpy2DAsync(pfx_tok, (size_t)Le * 8, rq.pfx->tokens, (size_t)rq.pfx->ld * 8, (size_t)pfx_max * 8, rows,
                               hipMemcpyDeviceToDevice, s));
    if (rq.bm) {                                            // one prefix per sketch: in place, and the lengths through the area's second half
      if (pfx_max > 0) SKF_TRY(skf_beam_replicate(pfx_tok, pfx_tok, nsk, W, (size_t)2 * Le, s));
      SKF_HIP(hipMemcpyAsync(pfx_len + B, M->dec_pfx_len_host.data(), (size_t)nsk * sizeof(int), hipMemcpyHostToDevice, s));
      SKF_HIP(hipMemsetAsync(pfx_len, 0, (size_t)B * sizeof(int), s));         // (rows behind n W are not at work)
      SKF_TRY(skf_beam_replicate(pfx_len, pfx_len + B, nsk, W, 1, s));
    } else {
      SKF_HIP(hipMemcpyAsync(pfx_len, M->dec_pfx_len_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    }
    prefill = !rq.bm && !rq.pfx->stepwise && pfx_max > 0;
  }
  // pre_decoder and the cross-attention K/V of every layer: once
  if (V.emb)
    SKF_TRY(skf_expander_fwd(V.emb, M->P(L.exp_w), M->P(L.exp_b), B, Le, L.E, V.pre, s));
  for (int l = 0; l < N; ++l) {
    const DenseP& w = L.dec[l].mha2.kv;
    SKF_TRY(skf_gemm_f32(1, 0, B * Le, w.out, w.in, pre, w.in, M->P(w.w), w.ld, V.kv2[l], w.out, M->P(w.b), 0, nullptr, 0, 0, 1,
                         nullptr, 0, nullptr, 0, V.kv2_precision, s));
  }
  if (V.classify) {
    SKF_TRY(classify_fwd(M, false, s));                                                       // classify_from_embedding
    SKF_TRY(skf_softmax_ce(M->at<float>(P.cls_logits), c.n_classes, B, c.n_classes, M->at<long long>(P.labels), 1, 1, 0, 0, 0.f,
                           M->at<float>(P.cls_loss), M->at<float>(P.cls_hit), M->at<float>(P.cls_probs), 0, s));
  }
  return SKF_OK;
}

// One decode step, layer by layer (V.layerwise).  Every argument is the same for every step and every call (the step index,
// n_valid and eos are read from device memory), so the ~50 small launches are captured once into a hipGraph and replayed.
int DecodeRun::issue_step() {
  float* q = M->at<float>(P.dc_q); float* o = M->at<float>(P.dc_o); float* z = M->at<float>(P.dc_z);
  float* out1 = M->at<float>(P.dc_out1); float* out2 = M->at<float>(P.dc_out2); float* hbuf = M->at<float>(P.dc_h);
  float* stats = M->at<float>(P.dc_stats); float* logits = M->at<float>(P.dc_logits);
  float* kvnew = M->at<float>(P.dc_kvnew);
  float* x = M->at<float>(P.dc_x[0]);
  float* xn = M->at<float>(P.dc_x[1]);
  SKF_TRY(skf_decode_embed(tokens, cont, Ti, B, c.continuous ? nullptr : M->P(L.dec_emb), c.vocab_size,
                           c.continuous ? M->P(L.dec_embd.w) : nullptr, c.continuous ? M->P(L.dec_embd.b) : nullptr, d,
                           M->pos, step_dev, x, s));
  for (int l = 0; l < N; ++l) {
    const DecLayerP& w = L.dec[l];
    float* cache = V.cache[l];                                        // (B, Le, 2d): K | V of the positions so far
    const DenseP wq{w.mha1.qkv.w, w.mha1.qkv.b, d, d, w.mha1.qkv.ld};
    const DenseP wkv{w.mha1.qkv.w + d, w.mha1.qkv.b + d, d, 2 * d, w.mha1.qkv.ld};
    SKF_TRY(dense_fwd_ld(M, wq, x, d, B, q, d, 0, s));
    SKF_TRY(dense_fwd_ld(M, wkv, x, d, B, kvnew, 2 * d, 0, s));
    // keys 0..step: the cache plus the row just projected (which the kernel also appends to the cache)
    SKF_TRY(skf_attention_decode_w(q, d, cache, cache + d, 2 * d, (long long)Le * 2 * d, selfmask, Le + 1, nullptr, 0, B, H,
                                   Le, dh, o, d, step_dev, kvnew, kvnew + d, 2 * d, 0, rq.attn ? rq.attn + (size_t)(2 * l) * aw_blk : nullptr,
                                   rq.max_steps, Le, s));
    SKF_TRY(dense_fwd(M, w.mha1.o, o, B, z, 0, s));
    SKF_TRY(skf_layernorm_residual_fwd(x, z, M->P(w.ln1.g), M->P(w.ln1.b), out1, stats, B, d, 0.f, 0, M->state, s));
    const float* kv2 = V.kv2[l];
    SKF_TRY(dense_fwd(M, w.mha2.q, out1, B, q, 0, s));
    // cross mask (models/sketchformer.py:172,279-283): none when blind, else keys >= nattn (expected length or step+1)
    SKF_TRY(skf_attention_decode_w(q, d, kv2, kv2 + d, 2 * d, (long long)Le * 2 * d, nullptr, 0, limit, 0, B, H, Le, dh, o, d,
                                   step_dev, nullptr, nullptr, 0, c.blind_decoder_mask ? 0 : 1,
                                   rq.attn ? rq.attn + (size_t)(2 * l + 1) * aw_blk : nullptr, rq.max_steps, Le, s));
    SKF_TRY(dense_fwd(M, w.mha2.o, o, B, z, 0, s));
    SKF_TRY(skf_layernorm_residual_fwd(out1, z, M->P(w.ln2.g), M->P(w.ln2.b), out2, stats, B, d, 0.f, 0, M->state, s));
    SKF_TRY(dense_fwd(M, w.f1, out2, B, hbuf, 1, s));
    SKF_TRY(dense_fwd(M, w.f2, hbuf, B, z, 0, s));
    SKF_TRY(skf_layernorm_residual_fwd(out2, z, M->P(w.ln3.g), M->P(w.ln3.b), xn, stats, B, d, 0.f, 0, M->state, s));
    float* t = x; x = xn; xn = t;
  }
  SKF_TRY(dense_fwd(M, L.out, x, B, logits, 0, s));
  if (c.continuous)
    return skf_decode_select_continuous(logits, Vout, B, 0, 0, cont, Ti, selfmask, Le + 1, done_step, step_dev, dyn, s);
  if (rq.smp)
    return skf_decode_sample_tokens(logits, Vout, B, Vout, 0, 0, 0, tokens, Ti, selfmask, Le + 1, eos_seen, done_step, step_dev, dyn,
                                    rq.smp, stream_ids, s);
  return skf_decode_select_tokens(logits, Vout, B, Vout, 0, 0, 0, tokens, Ti, selfmask, Le + 1, eos_seen, done_step,
                                  step_dev, dyn, s);
}

int DecodeRun::fill_fused_params() {
  // One launch per position (skf_decode_fused.hip) unless SKF_MODEL_DECODE_LAYERWISE (skf_model_set_flags) asks for the layer-by-layer path above
  const bool fused_off = (M->flags & SKF_MODEL_DECODE_LAYERWISE) != 0;
  fused = rq.bm || !V.layerwise || (!fused_off && skf_decode_fused_supported(d, H, F, Le, N, Vout));
  if (fused) {
    auto dn = [&](const DenseP& w) {
      SkfDecDense r{M->P(w.w), M->P(w.b), w.in, w.out, w.ld, 0};
      r.vec4 = (w.ld & 3) == 0 && (w.out & 3) == 0 && ((uintptr_t)r.w & 15) == 0;
      return r;
    };
    fp.B = B; fp.Le = Le; fp.d = d; fp.H = H; fp.F = F; fp.N = N; fp.Vout = Vout; fp.vocab = c.vocab_size;
    fp.blind = c.blind_decoder_mask ? 1 : 0; fp.hs_len = F > Vout ? F : Vout;
    for (int l = 0; l < N; ++l) {
      const DecLayerP& w = L.dec[l];
      SkfDecLayer& o = fp.layer[l];
      o.qkv = dn(w.mha1.qkv); o.o = dn(w.mha1.o); o.q2 = dn(w.mha2.q); o.o2 = dn(w.mha2.o); o.f1 = dn(w.f1); o.f2 = dn(w.f2);
      o.ln1_g = M->P(w.ln1.g); o.ln1_b = M->P(w.ln1.b); o.ln2_g = M->P(w.ln2.g); o.ln2_b = M->P(w.ln2.b);
      o.ln3_g = M->P(w.ln3.g); o.ln3_b = M->P(w.ln3.b);
      o.cache = V.cache[l]; o.kv2 = V.kv2[l];
    }
    fp.out = dn(L.out);
    fp.emb_table = c.continuous ? nullptr : M->P(L.dec_emb);
    fp.embd_w = c.continuous ? M->P(L.dec_embd.w) : nullptr; fp.embd_b = c.continuous ? M->P(L.dec_embd.b) : nullptr;
    fp.pos = M->pos; fp.tokens = tokens; fp.cont = cont; fp.Ti = Ti; fp.selfmask = selfmask; fp.mask_ld = Le + 1;
    fp.eos_seen = eos_seen; fp.done_step = done_step; fp.step_dev = step_dev; fp.ticket = done_step + 1;
    fp.dyn = dyn; fp.limit = limit; fp.attn = rq.attn; fp.attn_rows = rq.max_steps;
    if (rq.smp) {
      fp.sample = 1; fp.temperature = rq.smp->temperature; fp.top_k = rq.smp->top_k; fp.top_p = rq.smp->top_p; fp.seed = rq.smp->seed;
      fp.stream_ids = stream_ids;
    }
    if (rq.bm) {
      fp.beam = W; fp.beam_rows = nsk * W; fp.anc = bs.anc; fp.cand_lp = bs.cand_lp; fp.cand_tok = bs.cand_tok;
    }
    if (rq.pfx) {
      fp.prefix = pfx_tok; fp.prefix_ld = Le; fp.prefix_len = pfx_len; fp.prefilled = prefill ? 1 : 0;
    }
    SKF_HIP(hipMemsetAsync(fp.ticket, 0, sizeof(int), s));
  }
  // the captured step has constant arguments, no weight output and the greedy selection: with weights requested or with
  // sampling, the steps are issued eagerly (g_dec stays as it is)
  use_graph = !fused && !rq.attn && !rq.smp && !rq.bm;
  return SKF_OK;
}

int DecodeRun::capture_step() {
  if (use_graph && !M->g_dec) {
    hipGraph_t graph = nullptr;
    SKF_HIP(hipStreamSynchronize(s));        // nothing of the setup above may end up inside the captured step
    SKF_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = issue_step();
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != SKF_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) { skf_set_error("hipStreamEndCapture (decode step): %s", hipGetErrorString(e)); return SKF_EHIP; }
    e = hipGraphInstantiate(&M->g_dec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { skf_set_error("hipGraphInstantiate (decode step): %s", hipGetErrorString(e)); M->g_dec = nullptr; return SKF_EHIP; }
  }
  return SKF_OK;
}

int DecodeRun::issue_position() {
  if (rq.bm) {
    SKF_TRY(skf_decode_fused_launch(fp, s));
    return skf_beam_advance_launch(bs, 0, 0, 0, s);      // (step, n_valid and eos come from device memory)
  }
  if (fused) return skf_decode_fused_launch(fp, s);
  if (!use_graph) return issue_step();
  SKF_HIP(hipGraphLaunch(M->g_dec, s));
  return SKF_OK;
}

int DecodeRun::decode_positions() {
  int done = -1, steps_run = 0, first = 0;
  if (prefill) {       // the cache rows of every forced position; the loop starts behind the prefix all rows share
    SKF_TRY(skf_decode_prefill_launch(fp, pfx_max, s));
    first = steps_run = pfx_min;
    if (first > 0) {   // the stop test of the positions skipped
      SKF_HIP(hipMemcpyAsync(&done, done_step, sizeof(int), hipMemcpyDeviceToHost, s));
      SKF_HIP(hipStreamSynchronize(s));
    }
  }
  for (int i = first; i < rq.max_steps && done < 0; ++i) {
    SKF_TRY(issue_position());
    steps_run = i + 1;
    if ((i & 7) == 7 || i + 1 == rq.max_steps) {            // the reference syncs every token; every 8th is enough here
      SKF_HIP(hipMemcpyAsync(&done, done_step, sizeof(int), hipMemcpyDeviceToHost, s));
      SKF_HIP(hipStreamSynchronize(s));
      if (done >= 0) break;
    }
  }
  const int ncols = (done >= 0 ? done + 1 : steps_run) + 1;     // start symbol + emitted positions
  if (rq.out_len_host) *rq.out_len_host = ncols;
  if (rq.bm) {      // after steps_run positions the current table is steps_run & 1; columns behind ncols are written as zeros
    SKF_TRY(skf_beam_gather(bs, steps_run & 1, ncols, T, rq.bm->length_alpha, rq.bm_out->tokens, rq.bm_out->scores, rq.bm_out->lengths, s));
    if (steps_run & 1)      // "decode/ancestry" is table 0: leave the table that was read there
      SKF_HIP(hipMemcpyAsync(bs.anc, bs.anc + (size_t)B * bs.anc_ld, (size_t)B * bs.anc_ld * sizeof(int), hipMemcpyDeviceToDevice, s));
    return SKF_OK;
  }
  // hand the valid columns to the caller's (B, max_steps + 1[, 5]) buffer
  const size_t esz = c.continuous ? 5 * sizeof(float) : sizeof(long long);
  SKF_HIP(hipMemcpy2DAsync(rq.out, (size_t)T * esz, c.continuous ? (const void*)cont : (const void*)tokens, (size_t)Ti * esz,
                           (size_t)ncols * esz, B, hipMemcpyDeviceToDevice, s));
  return SKF_OK;
}

}  // namespace

int run_decode(SkfModel* M, const DecodeRequest& rq, hipStream_t s) {
  DecodeRun R(M, rq, s);
  if (rq.pfx && !rq.bm && R.V.layerwise &&
      ((M->flags & SKF_MODEL_DECODE_LAYERWISE) || !skf_decode_fused_supported(R.d, R.H, R.F, R.Le, R.N, R.Vout))) {
    skf_set_error("a prefix is served by the one-launch position kernel only: not with SKF_MODEL_DECODE_LAYERWISE, nor at dimensions "
                  "that kernel does not take (d <= 512, <= 8 layers, head size 16 / 32 / 64)");
    return SKF_EUNSUPPORTED;
  }
  if (!R.V.layerwise)
    SKF_CHECK_ARG(skf_decode_fused_supported(R.d, R.H, R.F, R.Le, R.N, R.Vout), "greedy decode of a bf16 model needs the one-launch decoder (d <= 512, <= 8 layers)");
  SKF_TRY(R.decode_setup());
  SKF_TRY(R.fill_fused_params());
  SKF_TRY(R.capture_step());
  return R.decode_positions();
}
}  // namespace skf_model_detail
