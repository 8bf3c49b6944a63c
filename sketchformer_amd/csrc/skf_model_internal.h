// What the units of the train-step orchestrator share (included by the skf_model*.hip files only): the parameter layout and the two
// workspace plans, struct SkfModel, and the functions that cross a file boundary.  Those live in namespace skf_model_detail, out of
// the way of the skf_* launchers; what one unit alone uses stays in that unit's anonymous namespace.  A step's host state has three
// owners, one member of SkfModel each: SideSched (which stream, what waits for what), StepCtx (valid during one call only), ReduceBatch.
//   skf_model.hip          error slot, config, create / bind / destroy, input staging, graph capture, every skf_model_* entry
//   skf_model_prof.hip     the launch profiler
//   skf_model_layout.hip   parameter layout, workspace plans (fp32 and bf16), decode areas
//   skf_model_sched.hip    Dense helpers, the two-stream scheduler (SideSched), the batched reduction's bookkeeping (ReduceBatch)
//   skf_model_fwd.hip      fp32 forward                  skf_model_bwd.hip      fp32 backward, embedding sorts
//   skf_model_decode.hip   KV-cached reconstruction      skf_model_bf16.hip     the bf16 model's launch sequences
#pragma once
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>
#include <algorithm>
#include <functional>
#include "skf_common.h"
#include "skf_attention_params.h"
#include "skf_decode_fused.h"

namespace skf_model_detail {

struct DenseP { size_t w, b; int in, out, ld; };     // offsets into the flat buffer
struct LnP { size_t g, b; };
struct SelfMhaP { DenseP qkv, o; };
struct CrossMhaP { DenseP q, kv, o; };
struct EncLayerP { SelfMhaP mha; DenseP f1, f2; LnP ln1, ln2; };
struct DecLayerP { SelfMhaP mha1; CrossMhaP mha2; DenseP f1, f2; LnP ln1, ln2, ln3; };

// models/sketchformer.py:76-108: the bottleneck (+ expander) exists when lowerdim > 0, the class head only inside that
// block and only with do_classification, the decoder / output layer only with do_reconstruction
inline bool has_bott(const SkfConfig& c) { return c.lowerdim > 0; }
inline bool has_cls(const SkfConfig& c) { return c.lowerdim > 0 && c.do_classification != 0; }
inline bool do_recon(const SkfConfig& c) { return c.do_reconstruction != 0; }

struct Layout {
  size_t total = 0;
  size_t enc_emb = 0, dec_emb = 0;      // token mode: (V,d) tables
  DenseP enc_embd{}, dec_embd{};         // continuous mode: Dense(5 -> d)
  std::vector<EncLayerP> enc;
  std::vector<DecLayerP> dec;
  DenseP bott_w{};      // W_attn + b_attn
  size_t bott_v = 0;    // V_attn
  DenseP bott_e{};      // SelfAttnV2 only: Dense(lowerdim) after the pooling (builders/layers/transformer.py:92,128)
  std::vector<DenseP> cbuf;   // class_buffer Dense(lowerdim, relu) layers (models/sketchformer.py:101-104)
  size_t dec_off = 0;   // offset of the decoder embedding (== total when there is no decoder)
  int E = 0, Ua = 0;    // embedding width (d for V1, lowerdim for V2); units of the attention scorer (lowerdim / d)
  DenseP cls{}, out{};
  size_t exp_w = 0, exp_b = 0;
  std::vector<SkfParamEntry> entries;
};

// ------------------------------------------------------------------ workspace plan
struct Bump {
  size_t off = 0;
  size_t take(size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

// Scratch of the KV-cached reconstruction (run_decode), the same for both plans.  All fp32: the decoder of a bf16 model runs on the
// master weights.
struct DecodeAreas {
  size_t pre = 0;                 // own_cross plans only (bf16): the expanded embedding (B, L, d) ...
  std::vector<size_t> kv2;        // ... and the per-layer cross K|V (B, L, 2d); the fp32 plan decodes from its training buffers
  std::vector<size_t> cache;      // per-layer self-attention K|V of the positions so far (B, L, 2d)
  size_t img = 0;                 // the running output, (B, L + 1) tokens or stroke-5 rows: the step has constant arguments
  size_t mask = 0, flags = 0;     // self-attention padding mask (B, L + 1); [B] eos seen, done step, ticket
  size_t limit = 0;               // [B] key limits of the cross attention, then [B] stream ids of a sampled decode
  size_t dyn = 0;                 // per-call scalars + the step index
  // beam search (skf_beam.hip), rows g W + k: two ancestry tables (2, B, L + 1) ints; the W <= 8 candidates of a row, (B, 8) log p
  // then (B, 8) tokens; [B] scores, [B] finished flags, [B] lengths
  size_t anc = 0, cand = 0, beam = 0;
  // prefix-forced decoding: the prefix tokens (B, L) int64; [B] lengths, then [B] the lengths of a beam decode's sketches on their way
  // to the rows (the prefill keeps its intermediate rows in the caches themselves)
  size_t pfx_tok = 0, pfx_len = 0;
};

struct EncAct { size_t x_in, qkv, o, z1, st1, astats, x1, h, z2, st2, x2, hbits, img[2], img_o, img_qkv, img_of; };   // img: pre-split ffn weight images (forward, backward); img_o: Wo^T; img_qkv: this layer's Wqkv (read by the PREVIOUS layer's feed-forward launch)
struct DecAct { size_t x_in, qkv, o1, z1, st1, astats1, out1, q2, kv2, o2, astats2, z2, st2, out2, h, z3, st3, out3, hbits, img[2], img_o1, img_o2, img_qkv, img_o2f, img_o1f, img_q2, img_q2t; };

struct Plan {
  size_t bytes = 0;
  size_t inp, tar, labels, enc_mask, dec_mask;
  size_t order;            // (B) samples sorted by length, longest first (skf_sample_order): the attention launches deal their workgroups from it
  std::vector<EncAct> enc;
  std::vector<DecAct> dec;
  size_t u, pool_a, emb, pooled, dpooled, cls_logits, cls_probs, pre, logits;
  std::vector<size_t> cb_h, cb_f;       // class buffers: relu output, post-dropout output  (B, lowerdim) each
  size_t dcb[2];
  size_t recon_loss, recon_hit, cls_loss, cls_hit, row_mask, cont_scal;
  size_t gA, gB, gC, dqkv, dh, do_, dpre, dkv2, dq2, demb;
  // Buffers that weight-gradient GEMMs read (dY operands).  Two sets, alternating by layer: the wgrads of a layer are
  // issued together on the side stream at the end of that layer, so their operands must stay untouched until the
  // layer after next starts (every cross-stream event costs ~5 us of dead time on the main stream).
  struct GradSet { size_t dy[3], dh, dq2, dkv2, dqkv; };
  std::vector<GradSet> gs;        // gradient buffers of the backward, n_gs sets in rotation (one per layer where memory allows: see plan())
  int n_gs = 2;
  size_t gemm_ws, gemm_ws_bytes, small_ws, small_ws_bytes;
  size_t emb_sort[2] = {0, 0}, emb_sort_bytes = 0;         // token positions sorted by id (encoder, decoder): skf_embed_sort
  size_t slab_arena, slab_arena_bytes, descs, n_wgrads;   // deferred split-K reduction (eager path)
  size_t ln_part, ln_part_stride;                          // per-LayerNorm dgamma|dbeta partials [5N][g][2d], reduced in the same batch
  size_t bott_part = 0;                                    // expander / pooling gradient partials (see build_plan)
  // KV-cached decode (inference): the shared areas + the one-row-per-sample buffers of the layer-by-layer step (newest K|V rows last)
  DecodeAreas dca;
  size_t dc_x[2], dc_q, dc_o, dc_z, dc_out1, dc_out2, dc_h, dc_logits, dc_stats, dc_kvnew;
  size_t live_len = 0, live16 = 0, live32 = 0;   // decoder-side live rows of the step (token mode): per-sample count, block lists
};

// ------------------------------------------------------------------ bf16 workspace plan (skf_model_bf16.hip)
struct Img16 { size_t w = 0, wt = 0; int in = 0, out = 0, ld_src = 0, ldw = 0, ldt = 0; size_t src = 0; };
struct Enc16 { size_t x_in, qkv, o, olo, z1, st1, astats, x1, h, z2, st2, x2, hbits; };
struct Dec16 { size_t x_in, qkv, o1, olo1, z1, st1, astats1, out1, q2, kv2, o2, olo2, astats2, z2, st2, out2, h, z3, st3, out3, hbits; };

struct Plan16 {
  size_t bytes = 0;
  size_t inp = 0, tar = 0, labels = 0, enc_mask = 0, dec_mask = 0;
  std::vector<Enc16> enc;
  std::vector<Dec16> dec;
  size_t u = 0, pool_a = 0, emb = 0, cls_logits = 0, cls_probs = 0, pre = 0, logits = 0;
  int ld_logits = 0;
  size_t recon_loss = 0, recon_hit = 0, cls_loss = 0, cls_hit = 0;
  size_t gA = 0, gB = 0, dy = 0, dqkv = 0, dh = 0, dO = 0, dpre = 0, dkv2 = 0, dq2 = 0, demb = 0;
  size_t slab = 0, slab_bytes = 0, small_ws = 0, small_ws_bytes = 0, attn_ws = 0, attn_ws_bytes = 0, ln_ws = 0, ln_ws_bytes = 0;
  size_t cast_descs = 0, cast_descs_bytes = 0; int cast_n = 0, cast_blocks = 0; const float* cast_for = nullptr;   // weight-image descriptor table
  const char* tables_ws = nullptr;
  // LayerNorm gamma / beta gradients: every LayerNorm backward of the step leaves its [g][2d] partials in its own slab; two
  // batched reductions (decoder side, encoder side = the two gradient buckets) replace 80 small column-sum launches
  size_t ln_slabs = 0, ln_descs = 0; int ln_n = 0, ln_n_dec = 0, ln_blocks_dec = 0, ln_blocks_enc = 0, ln_cursor = 0; bool ln_batched = false;
  DecodeAreas dca;                                 // greedy / sampled reconstruction (fp32, on the master weights: run_decode)
  size_t order = 0;                                // samples sorted by length (skf_sample_order)
  size_t live_len = 0, live1 = 0, live64 = 0;      // live decoder rows of the step (skf_row_blocks.hip): row list, 64-row blocks
  size_t emb_sort[2] = {0, 0}, emb_sort_bytes = 0;
  std::map<size_t, Img16> img;          // keyed by DenseP.w (offset of the fp32 kernel in the flat buffer)
};

// ------------------------------------------------------------------ the step's batched reduction (skf_model_sched.hip)
// Bookkeeping of the ONE reduction launch per phase of the backward that sums the split-K slabs of the weight gradients, the
// LayerNorm dgamma|dbeta partials and the expander / pooling partials (flush_wgrads).  The launch sequence of a step is fixed: the
// descriptors are built on the first step, uploaded once, and only checked against on later steps.
struct ReduceBatch {
  std::vector<SkfReduceDesc> descs;     // one per wgrad of the step, in launch order
  bool descs_uploaded = false;
  size_t slab_cursor = 0, desc_cursor = 0, ln_cursor = 0;
  int reduce_blocks = 0;
  size_t phase_desc_begin = 0;          // first descriptor of the phase (gradient bucket) being issued
  bool side_used = false;

  void begin_step();                    // a backward starts: cursors to zero, the recorded descriptors stay
  void reset();                         // the launch sequence changes (skf_model_set_flags, skf_model_bind): the descriptors go as well
  // The next descriptor of the step, `blocks` workgroups of the reduction launch (d.block_begin == blocks()): recorded on the first
  // step, compared with the recorded one on later steps.
  int add(const SkfReduceDesc& d, int blocks);
  // This LayerNorm's slice of the partial arena / `bytes` of the slab arena with `queued` more descriptors still to come; null (and
  // the error text set) when the arena or the descriptor table is exhausted.
  float* take_ln_partial(SkfModel* M);
  float* take_slab(SkfModel* M, size_t bytes, size_t queued);
  // flush_wgrads: descriptors [begin, end) and `blocks` workgroups make up the phase's launch; end_phase starts the next one
  size_t begin() const { return phase_desc_begin; }
  size_t end() const { return desc_cursor; }
  int blocks() const { return reduce_blocks; }
  void end_phase(bool final);
};

// ------------------------------------------------------------------ the two-stream scheduler (skf_model_sched.hip)
// The ONE owner of what decides which stream a launch of the fp32 step goes to and what waits for what.  Weight-gradient GEMMs (and
// the input gradients nobody on the main stream needs soon) are queued per layer and issued as groups on the side stream, off the
// dgrad critical path; the main stream waits for a group only where it touches one of the group's buffers again.
struct SideSched {
  hipStream_t side = nullptr;           // null: the step runs on one stream (use_graph = 1, the bf16 model) and nothing is ever queued
  hipEvent_t fork_event = nullptr, join_event = nullptr;      // use_graph = 2: the side stream's entry into / exit from the capture
  std::vector<hipEvent_t> events;       // the pool every event between the two streams is taken from ...
  size_t next_event = 0;                // ... and its cursor
  // Side-stream events carry a sequence number (their record order on the in-order side stream): once the main stream has
  // waited for event k, every event <= k is complete too - later waits for those are dropped (a decoder layer's seven dY
  // buffers share one `done` event: one barrier packet on the main stream instead of seven, ~5 us each)
  struct SideEvent { hipEvent_t e; long seq; };
  long side_seq = 0, side_waited = 0;
  std::map<const void*, SideEvent> pending_readers;    // buffer -> completion event of its last side-stream reader
  std::map<const void*, SideEvent> pending_writers;    // buffers a side-stream dgrad still writes
  // kind 0: dW = X^T dY (+ bias grad); kind 1: an input gradient nobody on the main stream needs soon (dx (+)= dY W^T);
  // kind 2: one launch `run` that reads `dy` and whose result only the side stream consumes (the decoder embedding gradient)
  struct Queued { DenseP w; const float* x; int ldx; const float* dy; int lddy; int rows; int kind = 0; float* dx = nullptr; int lddx = 0; int accumulate = 0; const int* blocks32 = nullptr; std::function<int(hipStream_t)> run; };
  std::vector<Queued> wq;               // the current layer's group, not yet issued
  std::vector<Queued> wq_held;          // the PREVIOUS layer's group, held back until the next layer's first kernel is queued (hold)

  int create(bool captured);            // skf_model_create: the stream (+ the fork / join events of a captured two-stream step)
  void destroy();                       // skf_model_destroy: the pool, the fork / join events, the stream
  hipEvent_t take_event();              // the pool's next event (created on first use); null = allocation failed
  // The pool starts again at its first event.  Safe in the middle of a step because every event taken earlier in the call has been
  // waited for by then (a wait that is already enqueued keeps the record it saw: recording the event again does not move it).  Two
  // callers: run_forward in front of the decoder (the masks / images events were waited for in front of the first encoder layer)
  // and begin_backward (the forward's events were waited for by the side stream / in front of the first two cross-attentions).
  void rewind_events() { next_event = 0; }
  // A backward starts: the scheduler's start state - both queues and both pending maps empty, the pool rewound (whatever a backward
  // that returned early left behind goes here, nowhere else)
  void begin_backward() { wq.clear(); wq_held.clear(); pending_readers.clear(); pending_writers.clear(); rewind_events(); }
  void queue_wgrad(const DenseP& w, const float* x, int ldx, const float* dy, int lddy, int rows, const int* blocks32) { wq.push_back(Queued{w, x, ldx, dy, lddy, rows, 0, nullptr, 0, 0, blocks32}); }
  void queue_dgrad(const DenseP& w, const float* dy, int lddy, int rows, float* dx, int lddx, int accumulate) { wq.push_back(Queued{w, nullptr, 0, dy, lddy, rows, 1, dx, lddx, accumulate}); }
  void queue_launch(const float* reads, std::function<int(hipStream_t)> run) { Queued q{}; q.dy = reads; q.kind = 2; q.run = std::move(run); wq.push_back(std::move(q)); }
  bool holding() const { return !wq_held.empty(); }
  int hold(SkfModel* M, hipStream_t s);           // the queued group becomes the held one
  // The queued group goes out (behind the held one); ready_recorded: an event that already marks "the main stream is here" (the
  // completion signal of the launch in front of this call); on_main: the group runs on the main stream, in place
  int issue(SkfModel* M, hipStream_t s, hipEvent_t ready_recorded = nullptr, bool on_main = false);
  int issue_held(SkfModel* M, hipStream_t s, hipEvent_t ready_recorded = nullptr);
  // Main-stream kernels that overwrite `buf` first wait for the side-stream group that still reads it, those that read `buf` for the
  // deferred input gradient that still writes it (a group that is still queued or held is issued first)
  int before_write(SkfModel* M, const void* buf, hipStream_t s) { return wait_side(M, false, buf, s); }
  int before_read(SkfModel* M, const void* buf, hipStream_t s) { return wait_side(M, true, buf, s); }
  int wait_side(SkfModel* M, bool writers, const void* buf, hipStream_t s);
  int join(hipStream_t s);              // final flush: the main stream waits for everything on the side stream; nothing stays pending
  // use_graph = 2 (capture_or_run): the side stream enters the capture of `s` / is joined back before the capture ends
  bool fork_into_capture(hipStream_t s) { return hipEventRecord(fork_event, s) == hipSuccess && hipStreamWaitEvent(side, fork_event, 0) == hipSuccess; }
  bool join_capture(hipStream_t s) { return hipEventRecord(join_event, side) == hipSuccess && hipStreamWaitEvent(s, join_event, 0) == hipSuccess; }
};

// ------------------------------------------------------------------ what is valid during ONE call only
// Set by one function of a call and consumed by another; nothing here may survive into the next call on the model (whose batch has
// other live rows, whose events are other events).  reset() runs where the batch is staged (stage_inputs: every entry stages),
// begin_backward() at the entry of run_backward / run_backward16 for what a backward that returned early may have left set.
struct StepCtx {
  // Live rows of the decoder-side backward (skf_row_blocks.hip), set while the decoder layers' gradients are issued: a problem with
  // exactly `live_rows` rows walks the row-block list of its granule (fp32: 16 / 32 rows; bf16: single rows / 64), everything else
  // and every problem while no lists are set visits every row
  bool lists_set = false;
  int live_rows = 0;
  const int* live_len = nullptr;        // per-sample live length
  struct LiveList { int granule; const int* blocks; } lists[2] = {};
  const int* order = nullptr;           // this call's samples sorted by length (forward), or null
  hipEvent_t pre_ready = nullptr, masks_ready = nullptr;    // train step: forward_preamble ran on the side stream; the forward waits for the masks before its first attention, for the images behind it
  bool lists_built = false;             // this step's lists are in P.live16 / P.live32 (issued, not necessarily complete)
  bool masks_staged = false;            // the padding masks of this call were written by its staging launch (stage_inputs)
  bool ffn_fused = false;               // the feed-forward blocks run as one launch per direction (skf_ffn_fused.hip); set per forward
  bool metrics_deferred = false;        // train step, two streams, with a decoder: run_forward left skf_metrics_update to run_backward (side stream)
  hipEvent_t last_ready = nullptr;      // ffn_ln_bwd: the event attached to its fused launch (valid until the caller's next main-stream launch)

  void reset() { *this = StepCtx(); }
  void begin_backward() { clear_live(); last_ready = nullptr; }
  void set_live(int rows, const int* len, int g0, const int* b0, int g1, const int* b1) { lists_set = true; live_rows = rows; live_len = len; lists[0] = {g0, b0}; lists[1] = {g1, b1}; }
  void clear_live() { lists_set = false; live_rows = 0; live_len = nullptr; lists[0] = lists[1] = LiveList{}; }
  bool live(int rows) const { return lists_set && rows == live_rows; }
  const int* live_lengths(int rows) const { return live(rows) ? live_len : nullptr; }
  const int* live_blocks(int rows, int granule) const {
    return !live(rows) ? nullptr : lists[0].granule == granule ? lists[0].blocks : lists[1].granule == granule ? lists[1].blocks : nullptr;
  }
};

}  // namespace skf_model_detail

struct SkfModel {
  SkfConfig cfg;
  uint32_t flags = 0;                // skf_model_set_flags
  // sticky for the model's lifetime (not per call): a fused entry answered SKF_EUNSUPPORTED once, this model takes the general pair
  bool no_ln_fuse = false, no_relu_bits = false;
  skf_model_detail::StepCtx ctx;     // what is valid during one call only
  skf_model_detail::Layout lay;
  skf_model_detail::Plan plan;
  skf_model_detail::Plan16 p16;                        // bf16 path (cfg.act_dtype == SKF_ACT_BF16): its own workspace plan
  bool bf16 = false;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *metrics = nullptr;
  const float* pos = nullptr;
  char* ws = nullptr;
  void* state = nullptr;
  hipGraphExec_t g_fb = nullptr, g_opt = nullptr, g_dec = nullptr;   // g_dec: one greedy-decode step
  long long dec_dyn_host[2] = {0, 0};
  std::vector<int> dec_stream_host;  // stream ids of a sampled decode on their way to the device
  std::vector<int> dec_pfx_len_host; // prefix lengths of a completion on their way to the device
  float g_opt_scale = 0.f;
  // gradient clipping / monitoring (skf_model_set_gradient_clip): the settings, the regions of the caller's clip workspace and the
  // captured clipped step (g_clip, re-captured when grad_scale or a setting changes, like g_opt)
  struct Clip { bool on = false; int mode = 0, skip_nonfinite = 0, monitor = 0, n_chunks = 0; float threshold = 0.f, clipvalue = 0.f;
                float* stats = nullptr; void* plan = nullptr; void* norm_ws = nullptr; size_t norm_ws_bytes = 0; };
  Clip clip;
  hipGraphExec_t g_clip = nullptr;
  float g_clip_scale = 0.f;
  // weight averaging (skf_model_set_weight_average): the caller's shadow buffer and the rule of its update.  live: a swap has put the
  // average into `params` (and the raw weights into `shadow`) - the training entries refuse to run until a second swap
  struct Avg { float* shadow = nullptr; float decay = 0.f; int num_updates = 0; bool live = false; };
  Avg avg;
  skf_model_detail::SideSched sched;                   // the side stream and everything that orders the two streams
  hipEvent_t inputs_staged = nullptr;                         // recorded behind the staging copies of every call (skf_model_wait_inputs_staged)
  bool inputs_staged_valid = false;
  skf_model_detail::ReduceBatch red;                   // the batched reduction of the step's slabs and partials
  // gradient buckets (data parallelism): the flat gradient buffer becomes final in two pieces, in production order -
  // [dec_off, total) after the decoder backward, [0, dec_off) at the end; an event marks each piece complete so that
  // its all-reduce can start while the encoder backward / the previous piece's optimizer sweep still runs
  hipEvent_t bucket_ready[2] = {nullptr, nullptr};
  int n_buckets = 1;

  // the activations a caller may look at by name (skf_model_buffer / skf_model_buffer_info): filled by register_buffers(16)
  struct Named { size_t off; int rows, cols, ld, bf16; };
  std::map<std::string, Named> named;
  void reg(const std::string& name, size_t off, size_t rows, size_t cols, size_t ld, int is_bf16) {
    named[name] = {off, (int)rows, (int)cols, (int)ld, is_bf16};
  }

  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  float* P(size_t off) const { return params + off; }
  float* G(size_t off) const { return grads + off; }
};

#define SKF_TRY(call)            \
  do {                           \
    int rc__ = (call);           \
    if (rc__ != SKF_OK) return rc__; \
  } while (0)

namespace skf_model_detail {

extern thread_local int g_capturing;      // > 0 while this thread records a step into a hipGraph (capture_or_run; defined in skf_model.hip)

// site ids follow oracle.dropout_sites()
inline unsigned site_enc_embed() { return 0; }
inline unsigned site_enc(int layer, int j) { return 1 + 2 * layer + j; }
inline unsigned site_dec_embed(int N) { return 1 + 2 * N; }
inline unsigned site_class(int N, int i) { return 2 + 5 * N + i; }   // after the 1 + 2N encoder and 1 + 3N decoder sites
inline unsigned site_dec(int N, int layer, int j) { return 2 + 2 * N + 3 * layer + j; }

// Run `call` with event `e` riding on its LAST launch as that launch's completion signal instead of a packet of its own (skf_common.h:
// the attach protocol).  *rode = the launch carries it; false = the caller records `e` where it needs it.  Nothing is parked for a null
// `e`, while the step is being captured, or - the events that hand work to the side stream - without a side stream (`needs_side`).
inline bool may_park(const SkfModel* M, bool needs_side = true) { return !g_capturing && (M->sched.side || !needs_side); }
template <typename F>
int with_tail_event(SkfModel* M, hipEvent_t e, bool* rode, F call, bool needs_side = true) {
  SkfTailScope scope(may_park(M, needs_side) ? e : nullptr);
  const int rc = call();
  *rode = scope.attached();
  return rc;
}

// ------------------------------------------------------------------ skf_model_layout.hip
Layout build_layout(const SkfConfig& c);
bool decode_areas_ok(const DecodeAreas& A, size_t plan_bytes);
Plan build_plan(const SkfConfig& c);
Plan16 build_plan16(const SkfConfig& c, const Layout& L);

// ------------------------------------------------------------------ skf_model_sched.hip
int dense_fwd(SkfModel* M, const DenseP& w, const float* x, int rows, float* y, int act, hipStream_t s);
int dense_ln_fwd(SkfModel* M, const DenseP& w, const float* a, int rows, const float* x, float* z, const LnP& ln, float* out,
                 float* stats, float rate, unsigned site, hipStream_t s);
void* hbits_of(SkfModel* M, size_t off, int rows);
int dense_fwd_relu_bits(SkfModel* M, const DenseP& w, const float* x, int rows, float* y, void* bits, hipStream_t s);
int dense_fwd_ld(SkfModel* M, const DenseP& w, const float* x, int ldx, int rows, float* y, int ldy, int act, hipStream_t s);
int dense_wgrad(SkfModel* M, const DenseP& w, const float* x, int ldx, const float* dy, int lddy, int rows, hipStream_t s);
int flush_wgrads(SkfModel* M, hipStream_t s, int bucket, bool final, bool issue_queued = true, bool side_behind_main = false);
int dense_dgrad(SkfModel* M, const DenseP& w, const float* dy, int lddy, int rows, float* dx, int lddx, int accumulate,
                const float* relu_src, int ld_relu, hipStream_t s, const void* relu_bits = nullptr);
int dense_dgrad_deferred(SkfModel* M, const DenseP& w, const float* dy, int lddy, int rows, float* dx, int lddx, int accumulate,
                         hipStream_t s);

// ------------------------------------------------------------------ skf_model_fwd.hip, skf_model_bwd.hip
int classify_fwd(SkfModel* M, bool training, hipStream_t s);
int metrics_update(SkfModel* M, hipStream_t s);
int forward_preamble(SkfModel* M, bool with_backward, bool encoder_only, hipStream_t s, hipEvent_t masks_ready = nullptr);
int run_forward(SkfModel* M, bool training, bool with_loss, hipStream_t s, bool encoder_only = false);
int run_backward(SkfModel* M, hipStream_t s);
int issue_embed_sorts(SkfModel* M, hipStream_t s);

// ------------------------------------------------------------------ skf_model_decode.hip
// One reconstruction call.  Optional: attn (attention weights), smp + stream_ids_host (a sampled decode), bm + bm_out (beam search),
// pfx (a prefix to continue: sketch completion); see run_decode.
struct BeamOut { long long* tokens; float* scores; int* lengths; };
struct DecodeRequest {
  const float* embedding = nullptr;
  const int* expected_len_host = nullptr;
  int n_valid = 0;
  long long sos = 0, eos = 0;
  int max_steps = 0;
  void* out = nullptr;
  int* out_len_host = nullptr;
  float* attn = nullptr;
  const SkfSampling* smp = nullptr;
  const int* stream_ids_host = nullptr;
  const SkfBeam* bm = nullptr;
  const BeamOut* bm_out = nullptr;
  const SkfPrefix* pfx = nullptr;            // checked by the caller (prefix_check)
};
int run_decode(SkfModel* M, const DecodeRequest& rq, hipStream_t s);

// ------------------------------------------------------------------ skf_model_bf16.hip
void register_buffers16(SkfModel* M);
int ensure_cast_table16(SkfModel* M, hipStream_t s);
int run_forward16(SkfModel* M, bool training, bool with_loss, hipStream_t s, bool encoder_only = false);
int run_backward16(SkfModel* M, hipStream_t s);
int issue_embed_sorts16(SkfModel* M, hipStream_t s);
}  // namespace skf_model_detail
