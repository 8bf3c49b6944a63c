// Train-step orchestrator: the fixed launch sequence of Transformer.call +
// model_trainer (models/sketchformer.py:131-181, 325-349) over caller-owned flat
// device buffers, optionally captured into hipGraphs (one for forward+backward,
// one for the optimizer, so a data-parallel caller can all-reduce the flat
// gradient buffer in between).  No autograd: the backward sequence is explicit.
// This unit: the error slot, config, create / bind / destroy, input staging, graph capture and every skf_model_* entry; the launch
// sequences themselves are in the other skf_model_*.hip units (map in skf_model_internal.h).
#include "skf_model_internal.h"
using namespace skf_model_detail;

// ------------------------------------------------------------------ error plumbing
static thread_local char g_err[512] = "";
thread_local SkfTailSlot skf_tls_tail;      // skf_common.h: the event parked for this thread's next SKF_LAUNCH_TAIL launch
void skf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* skf_last_error(void) { return g_err; }
extern "C" int skf_version(void) { return 100; }
extern "C" int skf_device_info(char* name_host, size_t name_len, int* n_devices_host) {
  int n = 0;
  SKF_HIP(hipGetDeviceCount(&n));
  if (n_devices_host) *n_devices_host = n;
  if (name_host && name_len) {
    int dev = 0;
    SKF_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    SKF_HIP(hipGetDeviceProperties(&prop, dev));
    snprintf(name_host, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  return SKF_OK;
}

namespace skf_model_detail {
thread_local int g_capturing = 0;      // > 0 while this thread records a step into a hipGraph (capture_or_run)
}

namespace {

int prologue(SkfModel* M, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  return skf_step_prologue(M->state, c.schedule, c.sched_p0, c.sched_p1, c.sched_p2, c.sched_p3, c.beta1, c.beta2,
                           c.seed, s);
}

// Where a plan keeps the staged batch; masks: the two padding masks the staging launch may write as well (fp32 plan), or none
struct StageAreas { size_t inp, tar, labels; bool masks; size_t enc_mask, dec_mask; };

int stage_inputs(SkfModel* M, const StageAreas& P, const void* inp, const void* tar, int tar_ld, const long long* labels, hipStream_t s) {
  const SkfConfig& c = M->cfg;
  M->ctx.reset();      // every entry stages its batch: nothing of the previous call (an early error return included) reaches this one
  SKF_CHECK_ARG(inp && tar, "null input");
  const size_t row = c.continuous ? (size_t)c.seq_len * 5 * sizeof(float) : (size_t)c.seq_len * 8;     // bytes per sample
  const size_t src_row = c.continuous ? (size_t)tar_ld * 5 * sizeof(float) : (size_t)tar_ld * 8;
  // one launch for the three copies (skf_rowops.hip); operands that are not 4-byte aligned take the copy engine below
  // token mode: the two padding masks are written by the same launch (forward_preamble then skips its mask launches)
  const bool masks = P.masks && !c.continuous && tar_ld >= c.seq_len;
  const int rc = skf_stage_inputs_launch(inp, M->at<char>(P.inp), tar, M->at<char>(P.tar), row, src_row, row < src_row ? row : src_row, c.batch,
                                         labels, M->at<char>(P.labels), s, masks ? M->at<unsigned char>(P.enc_mask) : nullptr,
                                         masks ? M->at<unsigned char>(P.dec_mask) : nullptr, masks ? c.seq_len : 0);
  if (rc == SKF_OK) M->ctx.masks_staged = masks;
  if (rc != SKF_EUNSUPPORTED) return rc;
  SKF_HIP(hipMemcpyAsync(M->at<char>(P.inp), inp, row * c.batch, hipMemcpyDeviceToDevice, s));
  if (tar_ld == c.seq_len) {
    SKF_HIP(hipMemcpyAsync(M->at<char>(P.tar), tar, row * c.batch, hipMemcpyDeviceToDevice, s));
  } else {
    SKF_HIP(hipMemcpy2DAsync(M->at<char>(P.tar), row, tar, src_row, row < src_row ? row : src_row, c.batch,
                             hipMemcpyDeviceToDevice, s));
  }
  if (labels) SKF_HIP(hipMemcpyAsync(M->at<char>(P.labels), labels, (size_t)c.batch * 8, hipMemcpyDeviceToDevice, s));
  else SKF_HIP(hipMemsetAsync(M->at<char>(P.labels), 0, (size_t)c.batch * 8, s));
  return SKF_OK;
}

// The staging copies with the model's `inputs_staged` event behind them: a caller that hands over DEVICE tensors it will refill in place
// makes its own stream wait for that event (skf_model_wait_inputs_staged) instead of cloning the tensors in front of every call - the
// clones were two copy kernels on the caller's stream that the step then waited for, ~19 us of idle GPU at the head of every step.
// The event rides on the staging launch as its completion signal where there is one (SKF_LAUNCH_TAIL), else it is recorded.
template <typename F>
int stage_with_event(SkfModel* M, hipStream_t s, F stage) {
  if (!M->inputs_staged) SKF_HIP(hipEventCreateWithFlags(&M->inputs_staged, hipEventDisableTiming));
  // (runs in front of capture_or_run, never inside the library's own capture.  A caller whose stream is under a capture of ITS OWN
  //  would be detected here - hipStreamIsCapturing(s), then no parking - at the price of one more HIP call per step: not done)
  bool attached = false;
  SKF_TRY(with_tail_event(M, M->inputs_staged, &attached, stage, /*needs_side=*/false));
  if (!attached) SKF_HIP(hipEventRecord(M->inputs_staged, s));
  M->inputs_staged_valid = true;
  return SKF_OK;
}

// use_graph = 1: the step is captured on ONE stream (no side stream exists).  use_graph = 2 (round 5): the two-stream step is captured -
// the side stream joins the capture through an event recorded on the capturing stream (fork) and is joined back before the capture
// ends, so the weight-gradient groups / embedding sorts / K|V projections become parallel branches of the graph.  The first call runs
// eagerly: it builds and uploads the reduction descriptors (a synchronous copy, not capturable) that the captured sequence reuses.
template <typename F>
int capture_or_run(SkfModel* M, hipGraphExec_t* exec, hipStream_t s, F body) {
  if (!M->cfg.use_graph) return body();
  // use_graph = 2 replays a MULTI-BRANCH graph, and hipGraphLaunch of such a graph reads past the end of the exec's stream vector in the
  // HIP runtime whenever one of the exec's internal streams compares equal to the launch stream (hip::Graph::UpdateStreams: analysis in
  // include/skf.h at SKF_MODEL_TWO_STREAM_GRAPH, DESIGN.md section 6 "Round 6").  Whether that happens is decided by the runtime's state
  // in the PROCESS, so the mode needs the caller's explicit SKF_MODEL_TWO_STREAM_GRAPH; without it the same launches go out eagerly on
  // the two streams (bit-equal results, and the faster form anyway).
  if (M->cfg.use_graph == 2 && !(M->flags & SKF_MODEL_TWO_STREAM_GRAPH)) return body();
  const bool two_stream = M->sched.side != nullptr && exec == &M->g_fb;
  if (two_stream && !M->red.descs_uploaded) return body();
  if (!*exec) {
    hipGraph_t graph = nullptr;
    SKF_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    ++g_capturing;
    int rc = SKF_OK;
    if (two_stream && !M->sched.fork_into_capture(s)) rc = SKF_EHIP;
    if (rc == SKF_OK) rc = body();
    if (two_stream && rc == SKF_OK && !M->sched.join_capture(s)) rc = SKF_EHIP;
    --g_capturing;
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != SKF_OK) { if (graph) (void)hipGraphDestroy(graph); if (rc == SKF_EHIP) skf_set_error("two-stream capture: fork / join failed"); return rc; }
    if (e != hipSuccess) { skf_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return SKF_EHIP; }
    e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { skf_set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); *exec = nullptr; return SKF_EHIP; }
  }
  SKF_HIP(hipGraphLaunch(*exec, s));
  return SKF_OK;
}

}  // namespace

// =========================================================================== C ABI
extern "C" size_t skf_config_size(void) { return sizeof(SkfConfig); }

extern "C" int skf_model_set_flags(SkfModel* M, uint32_t flags) {
  SKF_CHECK_ARG(M, "null model");
  SKF_CHECK_ARG((flags & ~(SKF_MODEL_DECODE_LAYERWISE | SKF_MODEL_FFN_LAUNCHES | SKF_MODEL_TWO_STREAM_GRAPH)) == 0, "unknown flag bits");
  // SKF_MODEL_FFN_LAUNCHES changes the launch sequence of the step, hence the split counts of the LayerNorm partials and the
  // reduction descriptors that were built (and uploaded once) by the first step, and the captured step graphs: drop them like
  // skf_model_bind does, so that the next step rebuilds its descriptors / re-captures with the new sequence.
  if ((M->flags ^ flags) & SKF_MODEL_FFN_LAUNCHES) {
    SKF_HIP(hipDeviceSynchronize());     // steps in flight still read the descriptor table the next step uploads again
    if (M->g_fb) { (void)hipGraphExecDestroy(M->g_fb); M->g_fb = nullptr; }
    if (M->g_opt) { (void)hipGraphExecDestroy(M->g_opt); M->g_opt = nullptr; }
    if (M->g_clip) { (void)hipGraphExecDestroy(M->g_clip); M->g_clip = nullptr; }
    M->red.reset();
  }
  M->flags = flags;
  return SKF_OK;
}

extern "C" int skf_config_validate(const SkfConfig* c) {
  SKF_CHECK_ARG(c, "null config");
  if (c->struct_size != sizeof(SkfConfig)) {
    skf_set_error("SkfConfig.struct_size is %u, this library's SkfConfig has %zu bytes: the caller's declaration of the struct does not "
                  "match include/skf.h (set struct_size = sizeof(SkfConfig))", c->struct_size, sizeof(SkfConfig));
    return SKF_EINVAL;
  }
  SKF_CHECK_ARG(c->batch > 0 && c->seq_len > 1 && c->num_layers > 0, "bad sizes");
  SKF_CHECK_ARG(c->d_model % c->num_heads == 0, "d_model must be divisible by num_heads");
  const int dh = c->d_model / c->num_heads;
  // Any d_model % num_heads == 0 like the reference (builders/layers/transformer.py:150-152).  The MFMA kernels serve d_model in
  // {64,128,256,512} with head sizes {16,32,64} (every BASELINE config); other shapes run on the plain fp32 kernels of
  // skf_generic.hip (LayerNorm, expander, attention) and the generic GEMM.  Limits of those: d_model % 4 == 0 and
  // head size % 4 == 0 (16-byte rows and head slices), d_model <= 1024, head size <= 128.
  if ((c->d_model & 3) || c->d_model > 1024 || dh > 128 || (dh & 3)) {
    skf_set_error("d_model %d / head size %d: need d_model %% 4 == 0, d_model <= 1024, head size %% 4 == 0, head size <= 128", c->d_model, dh);
    return SKF_EUNSUPPORTED; }
  SKF_CHECK_ARG(c->attn_version == 1 || c->attn_version == 2, "attn_version must be 1 (SelfAttnV1) or 2 (SelfAttnV2)");
  SKF_CHECK_ARG(c->lowerdim >= 0, "lowerdim must be >= 0");
  // models/sketchformer.py:96-108,338: the class head only exists with a bottleneck; asking for it without one fails
  // in the reference too (the 'class' loss is never registered)
  SKF_CHECK_ARG(c->lowerdim > 0 || !c->do_classification, "do_classification needs lowerdim > 0");
  SKF_CHECK_ARG(c->do_reconstruction || (c->lowerdim > 0 && c->do_classification), "nothing to train: no decoder and no class head");
  if (c->lowerdim > 0 && c->attn_version == 2 && ((c->lowerdim & 3) || c->lowerdim > 1024)) {
    skf_set_error("attn_version=2: lowerdim %d (the embedding width) must be a multiple of 4, at most 1024", c->lowerdim); return SKF_EUNSUPPORTED; }
  SKF_CHECK_ARG(c->class_buffer_layers >= 0 && c->class_buffer_layers <= 8, "class_buffer_layers must be in [0, 8]");
  SKF_CHECK_ARG(c->class_dropout >= 0.f && c->class_dropout < 1.f, "class_dropout out of range");
  SKF_CHECK_ARG(c->optimizer == 0 || c->optimizer == 1, "optimizer must be 0 (Adam) or 1 (SGD with momentum)");
  SKF_CHECK_ARG(c->gemm_precision == SKF_PREC_F32 || c->gemm_precision == SKF_PREC_BF16X3 || c->gemm_precision == SKF_PREC_BF16X6,
                "gemm_precision must be 0 (fp32 MFMA), 6 (bf16x6) or 3 (bf16x3)");
  SKF_CHECK_ARG(c->n_classes > 0, "bad number of classes");
  if (!c->continuous) {
    SKF_CHECK_ARG(c->vocab_size > 0, "bad vocab size");
    SKF_CHECK_ARG(c->vocab_size % 4 == 0, "vocab_size must be a multiple of 4");
  }
  SKF_CHECK_ARG(c->dff % 4 == 0 && c->lowerdim % 4 == 0, "dff and lowerdim must be multiples of 4");
  SKF_CHECK_ARG(c->max_pos >= c->seq_len, "max_pos < seq_len");
  SKF_CHECK_ARG(c->dropout_rate >= 0.f && c->dropout_rate < 1.f, "dropout_rate out of range");
  SKF_CHECK_ARG(c->seq_len <= 512, "seq_len > 512 not supported");
  SKF_CHECK_ARG(c->act_dtype == SKF_ACT_F32 || c->act_dtype == SKF_ACT_BF16, "act_dtype must be 0 (fp32) or 1 (bf16)");
  if (c->act_dtype == SKF_ACT_F32 && (dh == 16 || dh == 32 || dh == 64)) {
    // the fp32 MFMA attention kernels keep one head's K / V (forward) or Q / dO (backward) in LDS: the encoder calls have
    // Lq = Lk = seq_len, and a model whose first step a launch would refuse is refused here (same size functions)
    const int fmax = skf_attention_fwd_max_lk(dh, c->gemm_precision), bmax = skf_attention_bwd_max_lq(dh);
    const bool bwd2 = dh == 32 && c->gemm_precision != SKF_PREC_F32 && c->seq_len <= 256;     // (the two-pass kernel's own footprint)
    if (c->seq_len > fmax || c->seq_len > bmax || (bwd2 && skf_attention_bwd2_smem(dh, c->seq_len, c->seq_len) > kAttnLdsBytes)) {
      skf_set_error("head size %d: seq_len %d does not fit the fp32 attention kernels (forward: at most %d keys, backward: at most %d query rows)",
                    dh, c->seq_len, fmax, bmax);
      return SKF_EUNSUPPORTED;
    }
  }
  if (c->act_dtype == SKF_ACT_BF16) {
    // the bf16 path is built for the default structure of the model (what BASELINE cfg 5 trains)
    if (c->continuous || c->attn_version != 1 || c->lowerdim <= 0 || !c->do_classification || !c->do_reconstruction ||
        c->class_buffer_layers != 0) {
      skf_set_error("act_dtype=bf16 supports token mode with attn_version=1, bottleneck + classifier + decoder, no class buffers");
      return SKF_EUNSUPPORTED;
    }
    if (dh != 64) { skf_set_error("act_dtype=bf16: head size %d, the streaming attention kernels are built for 64", dh); return SKF_EUNSUPPORTED; }
    if (!(c->d_model == 128 || c->d_model == 256 || c->d_model == 512)) { skf_set_error("act_dtype=bf16: d_model %d not in {128,256,512}", c->d_model); return SKF_EUNSUPPORTED; }
    SKF_CHECK_ARG(c->dff % 8 == 0 && c->lowerdim % 8 == 0, "act_dtype=bf16: dff and lowerdim must be multiples of 8");
    SKF_CHECK_ARG(c->vocab_size <= 2040, "act_dtype=bf16: vocab_size > 2040 (the cross-entropy kernel keeps a row in registers)");
  }
  return SKF_OK;
}

extern "C" size_t skf_model_param_floats(const SkfConfig* cfg) {
  if (skf_config_validate(cfg) != SKF_OK) return 0;
  return build_layout(*cfg).total;
}

extern "C" int skf_model_param_entries(const SkfConfig* cfg, SkfParamEntry* out_host, int max_entries) {
  int rc = skf_config_validate(cfg);
  if (rc != SKF_OK) return rc;
  Layout L = build_layout(*cfg);
  const int n = (int)L.entries.size();
  if (out_host) for (int i = 0; i < n && i < max_entries; ++i) out_host[i] = L.entries[i];
  return n;
}

extern "C" size_t skf_model_workspace_bytes(const SkfConfig* cfg) {
  if (skf_config_validate(cfg) != SKF_OK) return 0;
  if (cfg->act_dtype == SKF_ACT_BF16) return build_plan16(*cfg, build_layout(*cfg)).bytes;
  return build_plan(*cfg).bytes;
}

namespace {
void register_buffers(SkfModel* M) {
  const SkfConfig& c = M->cfg;
  const Plan& P = M->plan;
  const size_t B = c.batch, L = c.seq_len, Ld = L - 1, d = c.d_model, N = c.num_layers, E = M->lay.E, F = c.dff;
  const size_t Vout = c.continuous ? 5 : (size_t)c.vocab_size;
  auto reg = [&](const std::string& n, size_t off, size_t rows, size_t cols) { M->reg(n, off, rows, cols, cols, 0); };
  reg("logits", P.logits, B * Ld, Vout);
  reg("class_probs", P.cls_probs, B, c.n_classes);
  reg("class_logits", P.cls_logits, B, c.n_classes);
  if (has_bott(c)) reg("embedding", P.emb, B, E);
  else reg("embedding", P.enc[N - 1].x2, B * L, d);              // no bottleneck: the encoder output (models/sketchformer.py:158-159)
  reg("enc_output", P.enc[N - 1].x2, B * L, d);
  reg("dec_output", P.dec[N - 1].out3, B * Ld, d);
  reg("pre_decoder", has_bott(c) ? P.pre : P.enc[N - 1].x2, B * L, E);
  reg("bottleneck_attn", P.pool_a, B, L);
  // the FFN hidden activations relu(x W1 + b1): parity tests read the ReLU branch taken on the device from them
  for (size_t i = 0; i < N; ++i) {
    reg("encoder/layer" + std::to_string(i) + "/ffn_h", P.enc[i].h, B * L, F);
    if (do_recon(c)) reg("decoder/layer" + std::to_string(i) + "/ffn_h", P.dec[i].h, B * Ld, F);
  }
  reg("enc_embed_out", P.enc[0].x_in, B * L, d);
  reg("dec_embed_out", P.dec[0].x_in, B * Ld, d);
}
}  // namespace

extern "C" int skf_model_create(const SkfConfig* cfg, SkfModel** out) {
  SKF_CHECK_ARG(out, "null out");
  int rc = skf_config_validate(cfg);
  if (rc != SKF_OK) return rc;
  SkfModel* M = new SkfModel();
  M->cfg = *cfg;
  M->lay = build_layout(*cfg);
  if (cfg->act_dtype == SKF_ACT_BF16) {
    M->bf16 = true;
    M->p16 = build_plan16(*cfg, M->lay);
    register_buffers16(M);
  } else {
    M->plan = build_plan(*cfg);
    register_buffers(M);
  }
  {   // the running image and the ancestry tables of the last reconstruction (4-byte words; see skf_model_beam_decode)
    const DecodeAreas& A = M->bf16 ? M->p16.dca : M->plan.dca;
    const size_t B = cfg->batch, L1 = cfg->seq_len + 1;
    if (!cfg->continuous) M->reg("decode/tokens", A.img, B, 2 * L1, 2 * L1, 0);
    M->reg("decode/ancestry", A.anc, B, L1, L1, 0);
    for (size_t l = 0; l < A.cache.size(); ++l)      // the self-attention K|V rows of the last reconstruction (see skf_model_prefix_decode)
      M->reg("decode/cache" + std::to_string(l), A.cache[l], B * cfg->seq_len, 2 * (size_t)cfg->d_model, 2 * (size_t)cfg->d_model, 0);
  }
  if (!decode_areas_ok(M->bf16 ? M->p16.dca : M->plan.dca, M->bf16 ? M->p16.bytes : M->plan.bytes)) {
    skf_set_error("skf_model_create: internal error, the %s plan's decode areas are not distinct allocations", M->bf16 ? "bf16" : "fp32");
    delete M;
    return SKF_EINVAL;
  }
  if (M->bf16) {
    // one stream; gradient buckets like the fp32 path (events cannot be recorded for outside waiters in a captured graph)
    if (!cfg->use_graph) {
      M->n_buckets = 2;
      for (int i = 0; i < 2; ++i) SKF_HIP(hipEventCreateWithFlags(&M->bucket_ready[i], hipEventDisableTiming));
    }
    *out = M;
    return SKF_OK;
  }
  // measured on MI355X: eager launches + a wgrad side stream beat hipGraph replay (graph nodes of different
  // streams do not overlap, 7.50 vs 7.72 ms/step), so the side stream is only used on the eager path
  // (round 5: use_graph = 2 captures the two-stream step - capture_or_run)
  if (cfg->use_graph != 1) SKF_TRY(M->sched.create(cfg->use_graph == 2));
  if (!cfg->use_graph) {     // events cannot be recorded for outside waiters inside a captured graph: one bucket there
    M->n_buckets = do_recon(*cfg) ? 2 : 1;
    for (int i = 0; i < 2; ++i) SKF_HIP(hipEventCreateWithFlags(&M->bucket_ready[i], hipEventDisableTiming));
  }
  *out = M;
  return SKF_OK;
}

extern "C" void skf_model_destroy(SkfModel* m) {
  if (!m) return;
  if (m->g_fb) (void)hipGraphExecDestroy(m->g_fb);
  if (m->g_opt) (void)hipGraphExecDestroy(m->g_opt);
  if (m->g_clip) (void)hipGraphExecDestroy(m->g_clip);
  if (m->g_dec) (void)hipGraphExecDestroy(m->g_dec);
  for (int i = 0; i < 2; ++i) if (m->bucket_ready[i]) (void)hipEventDestroy(m->bucket_ready[i]);
  if (m->inputs_staged) (void)hipEventDestroy(m->inputs_staged);
  m->sched.destroy();
  delete m;
}

extern "C" int skf_model_bind(SkfModel* m, float* params, float* grads, float* adam_m, float* adam_v, const float* pos,
                              void* workspace, size_t workspace_bytes, float* metrics, void* step_state) {
  SKF_CHECK_ARG(m && params && grads && adam_m && adam_v && pos && workspace && metrics && step_state, "null buffer");
  SKF_CHECK_ARG(workspace_bytes >= (m->bf16 ? m->p16.bytes : m->plan.bytes), "workspace too small");
  SKF_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  SKF_CHECK_ARG((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)adam_m | (uintptr_t)adam_v) & 15) == 0, "flat buffers must be 16-byte aligned");
  m->params = params; m->grads = grads; m->m = adam_m; m->v = adam_v; m->pos = pos;
  m->ws = (char*)workspace; m->metrics = metrics; m->state = step_state;
  if (m->g_fb) { (void)hipGraphExecDestroy(m->g_fb); m->g_fb = nullptr; }
  if (m->g_opt) { (void)hipGraphExecDestroy(m->g_opt); m->g_opt = nullptr; }
  if (m->g_clip) { (void)hipGraphExecDestroy(m->g_clip); m->g_clip = nullptr; }
  if (m->g_dec) { (void)hipGraphExecDestroy(m->g_dec); m->g_dec = nullptr; }
  m->red.reset();      // (the cursors as well: every backward starts them at zero anyway)
  return SKF_OK;
}

namespace {
// The batch into the plan's staging areas, with the `inputs_staged` event behind the copies (stage_with_event).  A bf16 model first makes
// sure its weight-image table is there, and its forward writes the padding masks itself.
int stage_batch(SkfModel* m, const void* inp, const void* tar, int tar_ld, const long long* labels, hipStream_t s) {
  return stage_with_event(m, s, [&]() -> int {
    if (!m->bf16) {
      const Plan& P = m->plan;
      return stage_inputs(m, {P.inp, P.tar, P.labels, true, P.enc_mask, P.dec_mask}, inp, tar, tar_ld, labels, s);
    }
    const Plan16& P = m->p16;
    SKF_TRY(ensure_cast_table16(m, s));
    return stage_inputs(m, {P.inp, P.tar, P.labels, false, 0, 0}, inp, tar, tar_ld, labels, s);
  });
}
}  // namespace

extern "C" int skf_model_forward(SkfModel* m, const void* inp, const void* tar, int tar_ld, int training,
                                 skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  hipStream_t s = (hipStream_t)stream;
  SKF_TRY(stage_batch(m, inp, tar, tar_ld, nullptr, s));
  if (training) SKF_TRY(prologue(m, s));
  return m->bf16 ? run_forward16(m, training != 0, false, s) : run_forward(m, training != 0, false, s);
}

extern "C" int skf_model_encode(SkfModel* m, const void* inp, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  hipStream_t s = (hipStream_t)stream;
  SKF_TRY(stage_batch(m, inp, inp, m->cfg.seq_len, nullptr, s));
  return m->bf16 ? run_forward16(m, false, false, s, true) : run_forward(m, false, false, s, true);
}

namespace {
// SkfPrefix as the completion entries take it (`rows` prefixes).  Decided from the configuration and the arguments alone, in front of
// everything that needs a bound model (a model that is not bound yet is told the same).
int prefix_check(const char* entry, const SkfModel* m, const SkfPrefix* pf, int rows, int max_steps) {
#define SKF_PFX_CHECK(cond, msg) \
  do { if (!(cond)) { skf_set_error("%s: %s (%s)", entry, msg, #cond); return SKF_EINVAL; } } while (0)
  SKF_PFX_CHECK(m, "null model");
  SKF_PFX_CHECK(pf, "null SkfPrefix");
  if (m->cfg.continuous) {
    skf_set_error("%s: a prefix is a sequence of tokens forced on the one-launch position kernel: continuous (stroke-5) prefixes are not built",
                  entry);
    return SKF_EUNSUPPORTED;
  }
  SKF_PFX_CHECK(max_steps > 0 && max_steps <= m->cfg.seq_len, "max_steps must be in [1, seq_len]");
  if (pf->struct_size != sizeof(SkfPrefix)) {
    skf_set_error("%s: SkfPrefix.struct_size is %u, this library's SkfPrefix has %zu bytes (set struct_size = sizeof(SkfPrefix))", entry,
                  pf->struct_size, sizeof(SkfPrefix));
    return SKF_EINVAL;
  }
  SKF_PFX_CHECK(pf->tokens && pf->len_host, "null prefix tokens or lengths");
  SKF_PFX_CHECK(rows > 0 && max_steps > 0, "no rows or no positions");
  for (int r = 0; r < rows; ++r) {
    SKF_PFX_CHECK(pf->len_host[r] >= 0 && pf->len_host[r] <= max_steps, "a prefix length must be in [0, max_steps]");
    SKF_PFX_CHECK(pf->len_host[r] <= pf->ld, "ld must not be smaller than the longest prefix");
  }
#undef SKF_PFX_CHECK
  return SKF_OK;
}

// The reconstruction entries.  `entry` names the caller in the error text; sampled: skf_model_sample_decode (tokens are drawn);
// rq: skf_model_beam_decode hands in its beam members (out = the tokens of rq.bm_out), the rest of the request is filled here.
int decode_entry(const char* entry, SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                 long long eos, int max_steps, void* out, int* out_len_host, float* attn_weights, bool sampled,
                 const SkfSampling* sampling, const int* stream_ids_host, skf_stream_t stream, DecodeRequest rq = DecodeRequest()) {
#define SKF_ENTRY_CHECK(cond, msg) \
  do { if (!(cond)) { skf_set_error("%s: %s (%s)", entry, msg, #cond); return SKF_EINVAL; } } while (0)
  SKF_ENTRY_CHECK(m && m->ws, "model not bound");
  SKF_ENTRY_CHECK(out, "null output");
  SKF_ENTRY_CHECK(n_valid > 0 && n_valid <= m->cfg.batch, "n_valid must be in [1, batch]");
  SKF_ENTRY_CHECK(max_steps > 0 && max_steps <= m->cfg.seq_len, "max_steps must be in [1, seq_len]");
  SKF_ENTRY_CHECK(m->cfg.do_reconstruction, "the model was built without a decoder (do_reconstruction = 0)");
  if (rq.pfx && attn_weights) {      // (no public entry takes both)
    skf_set_error("%s: the attention weights of a completion are not built", entry);
    return SKF_EUNSUPPORTED;
  }
  SKF_ENTRY_CHECK(!attn_weights || m->cfg.blind_decoder_mask || expected_len_host,
                  "attention weights of a non-blind decoder need expected_len (with nattn = i + 1 the cached rows differ from the "
                  "reference's last pass)");
#undef SKF_ENTRY_CHECK
  if (sampled) {
    SKF_TRY(skf_sampling_check(sampling));
    if (m->cfg.continuous) {
      skf_set_error("skf_model_sample_decode: a continuous model has a regression head and three pen logits, no categorical distribution "
                    "over tokens to draw from: sampled decoding is built for token models only");
      return SKF_EUNSUPPORTED;
    }
  }
  rq.embedding = embedding; rq.expected_len_host = expected_len_host; rq.n_valid = n_valid; rq.sos = sos; rq.eos = eos;
  rq.max_steps = max_steps; rq.out = out; rq.out_len_host = out_len_host; rq.attn = attn_weights;
  rq.smp = sampled ? sampling : nullptr; rq.stream_ids_host = stream_ids_host;
  return run_decode(m, rq, (hipStream_t)stream);
}

// skf_model_beam_decode, and with `prefix` skf_model_beam_prefix_decode
int beam_entry(const char* entry, SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
               long long eos, int max_steps, long long* out_tokens, float* out_scores, int* out_lengths, int* out_len_host,
               const SkfBeam* beam, const SkfPrefix* prefix, skf_stream_t stream) {
  // what depends on the configuration alone is answered first (a model that is not bound yet is told the same)
#define SKF_BEAM_CHECK(cond, msg) \
  do { if (!(cond)) { skf_set_error("%s: %s (%s)", entry, msg, #cond); return SKF_EINVAL; } } while (0)
  SKF_BEAM_CHECK(m, "null model");
  SKF_TRY(skf_beam_check(beam));
  const SkfConfig& c = m->cfg;
  SKF_BEAM_CHECK(!c.continuous, "a continuous model decodes one deterministic stroke-5 row per position, with nothing to rank: "
                                "beam search is built for token models only");
  SKF_BEAM_CHECK(c.do_reconstruction, "the model was built without a decoder (do_reconstruction = 0)");
  SKF_BEAM_CHECK(beam->beam_width <= c.vocab_size && beam->beam_width <= c.batch, "beam_width must be in [1, min(8, vocab_size, batch)]");
  SKF_BEAM_CHECK(n_valid >= 1 && n_valid <= c.batch / beam->beam_width, "n_valid must be in [1, batch / beam_width]");
  SKF_BEAM_CHECK(skf_decode_beam_supported(c.d_model, c.num_heads, c.dff, c.seq_len, c.num_layers, c.vocab_size) &&
                     (unsigned long long)c.batch * c.seq_len * 2 * c.d_model < (1ull << 32),
                 "beam search needs the one-launch decoder with room for its ancestry row (d <= 512, <= 8 layers, head size 16 / 32 / 64)");
  SKF_BEAM_CHECK(c.blind_decoder_mask || expected_len_host, "beam search of a non-blind decoder needs expected_len");
  SKF_BEAM_CHECK(embedding && out_tokens && out_scores && out_lengths, "null embedding or output");
#undef SKF_BEAM_CHECK
  if (prefix) SKF_TRY(prefix_check(entry, m, prefix, c.batch / beam->beam_width, max_steps));
  const BeamOut bo{out_tokens, out_scores, out_lengths};
  DecodeRequest rq;
  rq.bm = beam; rq.bm_out = &bo; rq.pfx = prefix;
  return decode_entry(entry, m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out_tokens, out_len_host, nullptr, false,
                      nullptr, nullptr, stream, rq);
}
}  // namespace

extern "C" int skf_model_beam_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                                     long long eos, int max_steps, long long* out_tokens, float* out_scores, int* out_lengths,
                                     int* out_len_host, const SkfBeam* beam, skf_stream_t stream) {
  return beam_entry(__func__, m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out_tokens, out_scores, out_lengths,
                    out_len_host, beam, nullptr, stream);
}

extern "C" int skf_model_beam_prefix_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                                            long long eos, int max_steps, long long* out_tokens, float* out_scores, int* out_lengths,
                                            int* out_len_host, const SkfBeam* beam, const SkfPrefix* prefix, skf_stream_t stream) {
  if (!prefix) { skf_set_error("%s: null SkfPrefix", __func__); return SKF_EINVAL; }
  return beam_entry(__func__, m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out_tokens, out_scores, out_lengths,
                    out_len_host, beam, prefix, stream);
}

extern "C" int skf_model_prefix_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                                       long long eos, int max_steps, void* out, int* out_len_host, const SkfPrefix* prefix,
                                       const SkfSampling* sampling, const int* stream_ids_host, skf_stream_t stream) {
  SKF_TRY(prefix_check(__func__, m, prefix, m ? m->cfg.batch : 0, max_steps));
  DecodeRequest rq;
  rq.pfx = prefix;
  return decode_entry(__func__, m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out, out_len_host, nullptr,
                      sampling != nullptr, sampling, stream_ids_host, stream, rq);
}

extern "C" int skf_model_greedy_decode_attn(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid,
                                            long long sos, long long eos, int max_steps, void* out, int* out_len_host,
                                            float* attn_weights, skf_stream_t stream) {
  return decode_entry(__func__, m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out, out_len_host, attn_weights, false,
                      nullptr, nullptr, stream);
}

extern "C" int skf_model_sample_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid,
                                       long long sos, long long eos, int max_steps, void* out, int* out_len_host,
                                       const SkfSampling* sampling, const int* stream_ids_host, skf_stream_t stream) {
  return decode_entry(__func__, m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out, out_len_host, nullptr, true, sampling,
                      stream_ids_host, stream);
}

extern "C" int skf_model_greedy_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid,
                                       long long sos, long long eos, int max_steps, void* out, int* out_len_host,
                                       skf_stream_t stream) {
  return skf_model_greedy_decode_attn(m, embedding, expected_len_host, n_valid, sos, eos, max_steps, out, out_len_host, nullptr,
                                      stream);
}

// what the training entries answer while a swap has the weight average in `params` (skf_model_swap_weight_average): a step would
// train the average and leave the raw weights behind in the shadow
static const char kAvgLive[] = "the weight average is live in `params` (skf_model_swap_weight_average): swap back before training";

extern "C" int skf_model_forward_backward(SkfModel* m, const void* inp, const void* tar, int tar_ld,
                                          const long long* labels, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(!m->avg.live, kAvgLive);
  SKF_CHECK_ARG(labels, "null labels");
  hipStream_t s = (hipStream_t)stream;
  SKF_TRY(stage_batch(m, inp, tar, tar_ld, labels, s));
  if (m->bf16) {
    return capture_or_run(m, &m->g_fb, s, [&]() -> int {
      SKF_TRY(prologue(m, s));
      SKF_TRY(issue_embed_sorts16(m, s));
      SKF_TRY(run_forward16(m, true, true, s));
      return run_backward16(m, s);
    });
  }
  return capture_or_run(m, &m->g_fb, s, [&]() -> int {
    SKF_TRY(prologue(m, s));
    SKF_TRY(issue_embed_sorts(m, s));
    SKF_TRY(run_forward(m, true, true, s));
    return run_backward(m, s);
  });
}

extern "C" int skf_model_wait_inputs_staged(SkfModel* m, skf_stream_t stream) {
  SKF_CHECK_ARG(m, "null model");
  SKF_CHECK_ARG(m->inputs_staged && m->inputs_staged_valid, "no call has staged inputs yet");
  SKF_HIP(hipStreamWaitEvent((hipStream_t)stream, m->inputs_staged, 0));
  return SKF_OK;
}

extern "C" int skf_model_apply_gradients(SkfModel* m, float grad_scale, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(!m->avg.live, kAvgLive);
  hipStream_t s = (hipStream_t)stream;
  if (m->g_opt && m->g_opt_scale != grad_scale) { (void)hipGraphExecDestroy(m->g_opt); m->g_opt = nullptr; }
  m->g_opt_scale = grad_scale;
  return capture_or_run(m, &m->g_opt, s, [&]() -> int {
    if (m->cfg.optimizer == 1)   // tf.keras.optimizers.SGD(lr_schedule, momentum) - the Adam m buffer is the velocity slot
      SKF_TRY(skf_sgd_momentum_step(m->params, m->grads, m->m, m->lay.total, m->state, grad_scale, m->cfg.momentum, s));
    else      // (the Adam sweep of a whole step also advances optimizer.iterations: one launch instead of two)
      return skf_adam_step_launch(m->params, m->grads, m->m, m->v, m->lay.total, m->state, grad_scale, m->cfg.beta1, m->cfg.beta2, m->cfg.eps, 1, s);
    return skf_step_epilogue(m->state, s);
  });
}

// ---- gradient clipping / monitoring (include/skf.h; kernels in skf_gradnorm.hip and skf_optimizer.hip)
namespace {
// the clip workspace: the stats words first (a caller reads them at offset 0), then the uploaded segment plan, then the scratch of the norms
struct ClipAreas { float* stats; void* plan; void* norm_ws; size_t plan_bytes, norm_ws_bytes, used; };
ClipAreas carve_clip(void* ws, int n_entries, int n_chunks) {
  SkfWsCarver c(ws);
  ClipAreas a;
  a.stats = c.take<float>(skf_segment_stats_floats(n_entries));
  a.plan_bytes = skf_segment_plan_bytes(n_entries, n_chunks);
  a.plan = c.take<char>(a.plan_bytes);
  a.norm_ws_bytes = skf_segment_norms_workspace_bytes(n_entries, n_chunks);
  a.norm_ws = c.take<char>(a.norm_ws_bytes);
  a.used = c.used;
  return a;
}
}  // namespace

extern "C" size_t skf_model_clip_workspace_bytes(const SkfConfig* cfg) {
  if (skf_config_validate(cfg) != SKF_OK) return 0;
  const Layout L = build_layout(*cfg);
  const int n_chunks = skf_segment_plan_chunks(L.entries.data(), (int)L.entries.size());
  if (n_chunks < 0) return 0;
  return carve_clip(nullptr, (int)L.entries.size(), n_chunks).used;
}

extern "C" int skf_model_set_gradient_clip(SkfModel* m, int mode, float threshold, float clipvalue, int skip_nonfinite, int monitor,
                                           void* workspace, size_t workspace_bytes) {
  SKF_CHECK_ARG(m, "null model");
  SKF_TRY(skf_gradient_clip_validate(mode, threshold, clipvalue));
  const bool on = mode != SKF_CLIP_NONE || clipvalue > 0.f || skip_nonfinite || monitor;
  SkfModel::Clip c;
  if (on) {
    const int E = (int)m->lay.entries.size();
    const int n_chunks = skf_segment_plan_chunks(m->lay.entries.data(), E);
    if (n_chunks < 0) return n_chunks;
    SKF_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0, "the clip workspace must be 256-byte aligned device memory");
    const ClipAreas a = carve_clip(workspace, E, n_chunks);
    SKF_CHECK_ARG(workspace_bytes >= a.used, "clip workspace too small (skf_model_clip_workspace_bytes)");
    std::vector<char> plan(a.plan_bytes);
    SKF_TRY(skf_segment_plan_build(m->lay.entries.data(), E, plan.data(), plan.size()));
    SKF_HIP(hipDeviceSynchronize());      // a step in flight may still read the old plan / write the old stats
    SKF_HIP(hipMemcpy(a.plan, plan.data(), plan.size(), hipMemcpyHostToDevice));
    std::vector<float> stats(skf_segment_stats_floats(E), 0.f);      // norms 0, counters 0, every scale 1
    stats[1] = 1.f;
    for (int e = 0; e < E; ++e) stats[8 + E + e] = 1.f;
    SKF_HIP(hipMemcpy(a.stats, stats.data(), stats.size() * sizeof(float), hipMemcpyHostToDevice));
    c.on = true; c.mode = mode; c.threshold = threshold; c.clipvalue = clipvalue; c.skip_nonfinite = skip_nonfinite != 0; c.monitor = monitor != 0;
    c.n_chunks = n_chunks; c.stats = a.stats; c.plan = a.plan; c.norm_ws = a.norm_ws; c.norm_ws_bytes = a.norm_ws_bytes;
  } else {
    SKF_HIP(hipDeviceSynchronize());
  }
  if (m->g_clip) { (void)hipGraphExecDestroy(m->g_clip); m->g_clip = nullptr; }
  m->clip = c;
  return SKF_OK;
}

extern "C" int skf_model_apply_gradients_clipped(SkfModel* m, float grad_scale, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(!m->avg.live, kAvgLive);
  SKF_CHECK_ARG(m->clip.on, "no gradient clip is configured (skf_model_set_gradient_clip); the plain sweep is skf_model_apply_gradients");
  hipStream_t s = (hipStream_t)stream;
  if (m->g_clip && m->g_clip_scale != grad_scale) { (void)hipGraphExecDestroy(m->g_clip); m->g_clip = nullptr; }
  m->g_clip_scale = grad_scale;
  return capture_or_run(m, &m->g_clip, s, [&]() -> int {
    const SkfModel::Clip& c = m->clip;
    const int E = (int)m->lay.entries.size();
    // clipvalue alone needs no reduction; everything else reads the norms / the skip decision
    const bool norms = c.mode != SKF_CLIP_NONE || c.skip_nonfinite || c.monitor;
    if (norms)
      SKF_TRY(skf_segment_norms(m->grads, c.plan, E, c.n_chunks, grad_scale, c.mode, c.threshold, c.skip_nonfinite, c.norm_ws, c.norm_ws_bytes,
                                c.stats, s));
    void* skip = norms ? (void*)(c.stats + 3) : nullptr;
    if (c.mode == SKF_CLIP_PER_VARIABLE) SKF_TRY(skf_segment_scale(m->grads, c.plan, E, c.n_chunks, c.stats + 8 + E, skip, s));
    const float* scale = c.mode == SKF_CLIP_GLOBAL ? c.stats + 1 : nullptr;
    if (m->cfg.optimizer == 1)      // (the Adam m buffer is the velocity slot)
      return skf_sgd_momentum_step_clipped(m->params, m->grads, m->m, m->lay.total, m->state, grad_scale, scale, c.clipvalue, skip,
                                           m->cfg.momentum, 1, s);
    return skf_adam_step_clipped(m->params, m->grads, m->m, m->v, m->lay.total, m->state, grad_scale, scale, c.clipvalue, skip, m->cfg.beta1,
                                 m->cfg.beta2, m->cfg.eps, 1, s);
  });
}

// ---- gradient accumulation (include/skf.h; the kernel is skf_accum.hip).  One eager launch per phase on the step's stream: the
// step graphs on either side read `grads` and the step state from device memory, so nothing captured changes with the phase.
extern "C" int skf_model_accumulate_gradients(SkfModel* m, float* acc, int phase, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(!m->avg.live, kAvgLive);
  SKF_CHECK_ARG(phase == SKF_ACCUM_FIRST || phase == SKF_ACCUM_ADD || phase == SKF_ACCUM_CLOSE || phase == SKF_ACCUM_RESET,
                "phase must be SKF_ACCUM_FIRST, _ADD, _CLOSE or _RESET");
  SKF_CHECK_ARG(acc || phase == SKF_ACCUM_RESET, "null accumulation buffer");
  const size_t n = m->lay.total;
  switch (phase) {
    case SKF_ACCUM_FIRST: return skf_grad_accumulate(acc, m->grads, nullptr, n, m->state, SKF_MICRO_NEXT, stream);
    case SKF_ACCUM_ADD:   return skf_grad_accumulate(acc, acc, m->grads, n, m->state, SKF_MICRO_NEXT, stream);
    case SKF_ACCUM_CLOSE: return skf_grad_accumulate(m->grads, acc, m->grads, n, m->state, SKF_MICRO_ZERO, stream);
    default:              return skf_grad_accumulate(nullptr, nullptr, nullptr, 0, m->state, SKF_MICRO_ZERO, stream);
  }
}

// ---- weight averaging (include/skf.h; the kernels are skf_ema.hip).  The update is one eager launch behind the sweep that advanced
// `iterations`; the swap exchanges the contents of `params` and the shadow - every forward rebuilds its weight images from `params`,
// so every entry point then runs on the average.
extern "C" int skf_model_set_weight_average(SkfModel* m, float* shadow, float decay, int num_updates) {
  SKF_CHECK_ARG(m, "null model");
  SKF_CHECK_ARG(!m->avg.live, "the weight average is live in `params`: swap back before changing or dropping the shadow");
  if (shadow) {
    SKF_TRY(skf_weight_average_validate(decay));
    SKF_CHECK_ARG(((uintptr_t)shadow & 15) == 0, "the shadow must be 16-byte aligned device memory");
  }
  SKF_HIP(hipDeviceSynchronize());      // an update in flight may still write the old shadow
  SkfModel::Avg a;
  if (shadow) { a.shadow = shadow; a.decay = decay; a.num_updates = num_updates != 0; }
  m->avg = a;
  return SKF_OK;
}

extern "C" int skf_model_update_weight_average(SkfModel* m, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(m->avg.shadow, "no weight average is configured (skf_model_set_weight_average)");
  SKF_CHECK_ARG(!m->avg.live, kAvgLive);
  const SkfModel::Clip& c = m->clip;
  const bool norms = c.on && (c.mode != SKF_CLIP_NONE || c.skip_nonfinite || c.monitor);      // as in skf_model_apply_gradients_clipped
  return skf_ema_update(m->avg.shadow, m->params, m->lay.total, m->avg.decay, m->avg.num_updates, m->state,
                        norms ? (const void*)(c.stats + 3) : nullptr, stream);
}

extern "C" int skf_model_swap_weight_average(SkfModel* m, skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(m->avg.shadow, "no weight average is configured (skf_model_set_weight_average)");
  SKF_TRY(skf_buffer_swap(m->params, m->avg.shadow, m->lay.total, stream));
  m->avg.live = !m->avg.live;
  return SKF_OK;
}

extern "C" int skf_model_weight_average_live(SkfModel* m) { return m && m->avg.live ? 1 : 0; }

extern "C" int skf_model_grad_buckets(SkfModel* m, int max_buckets, size_t* offsets_host, size_t* counts_host) {
  SKF_CHECK_ARG(m && offsets_host && counts_host && max_buckets >= 2, "bad argument");
  const size_t dec_off = m->lay.dec_off;
  if (m->n_buckets == 2) {
    offsets_host[0] = dec_off; counts_host[0] = m->lay.total - dec_off;      // decoder embedding .. output layer
    offsets_host[1] = 0; counts_host[1] = dec_off;                           // encoder .. expander
  } else {
    offsets_host[0] = 0; counts_host[0] = m->lay.total;
  }
  return m->n_buckets;
}

extern "C" int skf_model_wait_grad_bucket(SkfModel* m, int bucket, skf_stream_t stream) {
  SKF_CHECK_ARG(m && bucket >= 0 && bucket < m->n_buckets, "bad bucket");
  if (m->bucket_ready[bucket]) SKF_HIP(hipStreamWaitEvent((hipStream_t)stream, m->bucket_ready[bucket], 0));
  return SKF_OK;
}

extern "C" int skf_model_apply_gradients_range(SkfModel* m, size_t offset, size_t count, float grad_scale, int last,
                                               skf_stream_t stream) {
  SKF_CHECK_ARG(m && m->ws, "model not bound");
  SKF_CHECK_ARG(!m->avg.live, kAvgLive);
  SKF_CHECK_ARG((offset & 3) == 0 && offset + count <= m->lay.total, "range must start on a multiple of 4 floats inside the buffer");
  hipStream_t s = (hipStream_t)stream;
  if (count) {
    if (m->cfg.optimizer == 1)
      SKF_TRY(skf_sgd_momentum_step(m->params + offset, m->grads + offset, m->m + offset, count, m->state, grad_scale,
                                    m->cfg.momentum, s));
    else
      SKF_TRY(skf_adam_step(m->params + offset, m->grads + offset, m->m + offset, m->v + offset, count, m->state,
                            grad_scale, m->cfg.beta1, m->cfg.beta2, m->cfg.eps, s));
  }
  return last ? skf_step_epilogue(m->state, s) : SKF_OK;
}

extern "C" int skf_model_buffer_info(SkfModel* m, const char* name, void** ptr, int* rows, int* cols, int* ld, int* is_bf16) {
  SKF_CHECK_ARG(m && m->ws && name && ptr && rows && cols && ld && is_bf16, "bad argument");
  auto it = m->named.find(name);
  if (it == m->named.end()) {
    skf_set_error("%s: unknown buffer '%s'", m->bf16 ? "skf_model_buffer_info" : "skf_model_buffer", name);
    return SKF_EINVAL;
  }
  const SkfModel::Named& n = it->second;
  *ptr = m->ws + n.off; *rows = n.rows; *cols = n.cols; *ld = n.ld; *is_bf16 = n.bf16;
  return SKF_OK;
}

extern "C" int skf_model_buffer(SkfModel* m, const char* name, float** ptr, int* rows, int* cols) {
  SKF_CHECK_ARG(m && m->ws && name && ptr, "bad argument");
  auto it = m->named.find(name);
  if (m->bf16 && (it == m->named.end() || it->second.bf16)) {
    skf_set_error("skf_model_buffer: '%s' is not an fp32 buffer of this bf16 model (use skf_model_buffer_info)", name);
    return SKF_EINVAL;
  }
  if (it == m->named.end()) { skf_set_error("skf_model_buffer: unknown buffer '%s'", name); return SKF_EINVAL; }
  *ptr = m->at<float>(it->second.off);
  if (rows) *rows = it->second.rows;
  if (cols) *cols = it->second.cols;
  return SKF_OK;
}
