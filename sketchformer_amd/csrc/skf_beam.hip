// Beam-search reconstruction: everything around decode_position_kernel<.., BEAM> (skf_decode_fused.hip).
//
// A batch of B rows decodes n = B / W sketches; rows g W .. g W + W - 1 are the beams of sketch g.  A position is two launches:
// the position kernel (one workgroup per row: the decoder step, then the row's W best (log p, token) pairs) and
// beam_advance_kernel below (one wave per sketch: merge the W * W offers, keep the W best, write what the next position reads).
// No K/V row is ever copied: (row, position) is written once, at step == position, and a hypothesis is the list
// anc[r][0..step] of the slots that hold its history (two tables, read step & 1, written the other one).
//
// The selection rule (include/skf.h, restated in float64 by tests/beam_reference.py):
//   live beam r      offers (score[r] + logp[r][k], token[r][k]) for its W candidates k;
//   finished beam r  offers itself once: (score[r], PAD); its other W - 1 offers are -inf;
//   NaN ranks as -inf; the W best by score descending, then parent ascending, then token ascending (then offer index) survive.
// Scores are fp32 sums in step order; nothing here uses a floating-point atomic: the result is a pure function of the inputs.
#include "skf_common.h"
#include "skf_decode_fused.h"

namespace {

// dst row g W + k = src row g (k < W), rows of `cols` 4-byte words, rows walked from the last to the first by the thread that owns
// a column: a destination row never lies in front of its source row, so dst may be src (the model's own embedding buffer).
// One launch per decode call, n W <= B serial iterations per thread: nothing next to the decode itself; a 2-D grid with the
// in-place case apart is the form to take if that changes.  Rows >= n W of dst keep what they held: the expander, the cross K|V
// projections and the class head still run over all B rows, every row on its own, and nothing reads those rows' results.
__global__ __launch_bounds__(256) void beam_replicate_kernel(uint32_t* dst, const uint32_t* src, int n, int W, size_t cols) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  for (int r = n * W - 1; r >= 0; --r) dst[(size_t)r * cols + c] = src[(size_t)(r / W) * cols + c];
}

__global__ __launch_bounds__(256) void beam_init_kernel(SkfBeamState s) {
  for (int r = threadIdx.x; r < s.n * s.W; r += 256) {
    s.scores[r] = (r % s.W) == 0 ? 0.f : -INFINITY;      // the W beams start as one: beam 0 alone can offer
    s.finished[r] = 0;
    s.lengths[r] = 0;
    s.anc[(size_t)r * s.anc_ld] = r;                     // table 0, position 0: the start symbol of the row's own slot
  }
}

__global__ __launch_bounds__(64) void beam_advance_kernel(SkfBeamState s, int step, int n_valid, long long eos) {
  __shared__ int s_par[SKF_BEAM_MAX];
  const int g = blockIdx.x, lane = threadIdx.x, W = s.W, WW = W * W;
  if (s.step_dev) { step = *s.step_dev; n_valid = (int)s.dyn[0]; eos = s.dyn[1]; }
  const bool has = lane < WW;
  const int r = has ? lane / W : 0, k = lane - r * W;
  const int prow = g * W + r;
  // scores / finished / lengths are read here at the parent rows and written below, in place, at the survivor rows, with no barrier
  // between: right only because the block is ONE wave64 and every store depends on every lane's loads through the rank's shuffles.
  // A wider block, or stores moved in front of the rank, would need a second set of arrays.
  const float ps = s.scores[prow];
  const int pfin = s.finished[prow], plen = s.lengths[prow];
  float sc = -INFINITY;
  int tok = 0;
  if (has) {
    if (pfin) {
      if (k == 0) sc = ps;
    } else {
      sc = ps + s.cand_lp[(size_t)prow * W + k];
      tok = s.cand_tok[(size_t)prow * W + k];
    }
    if (!(sc == sc)) sc = -INFINITY;
  }
  int rank = 0;                                          // offers in front of this one
  for (int j = 0; j < WW; ++j) {
    const float os = __shfl(sc, j, 64);
    const int ot = __shfl(tok, j, 64), orr = j / W;
    const bool before = os > sc || (os == sc && (orr < r || (orr == r && (ot < tok || (ot == tok && j < lane)))));
    rank += before ? 1 : 0;
  }
  if (has && rank < W) {                                 // every rank below W * W is held by exactly one offer
    const int row = g * W + rank;
    s.tokens[(size_t)row * s.Ti + step + 1] = tok;
    s.selfmask[(size_t)row * s.mask_ld + step + 1] = tok == 0 ? 1 : 0;
    s.scores[row] = sc;
    s.finished[row] = (pfin || (long long)tok == eos) ? 1 : 0;
    s.lengths[row] = pfin ? plen : step + 1;
    s_par[rank] = r;
    if (s.parent) s.parent[row] = r;
  }
  __syncthreads();
  const int* tin = s.anc + (size_t)(step & 1) * s.B * s.anc_ld;
  int* tout = s.anc + (size_t)((step + 1) & 1) * s.B * s.anc_ld;
  for (int rr = 0; rr < W; ++rr) {
    const int* src = tin + (size_t)(g * W + s_par[rr]) * s.anc_ld;
    int* dst = tout + (size_t)(g * W + rr) * s.anc_ld;
    for (int j = lane; j <= step; j += 64) dst[j] = src[j];
    if (lane == 0) dst[step + 1] = g * W + rr;
  }
  if (!s.ticket) return;
  // ---- cross-sketch part, by whichever wave finishes the position last
  __threadfence();
  if (lane == 0) {
    const int t = atomicAdd(s.ticket, 1);
    if (t == (int)gridDim.x - 1) {
      __threadfence();
      int live = 0;
      for (int i = 0; i < n_valid * W; ++i) live += __hip_atomic_load(s.finished + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
      if (live == 0 && *s.done_step < 0) *s.done_step = step;
      if (s.step_dev) *s.step_dev = step + 1;
      *s.ticket = 0;
    }
  }
}

// The hypotheses of sketch g in their final order (score / ((5 + len) / 6)^alpha descending, then beam ascending), each read through
// its row of ancestry table `table`: out_tokens (n, W, T), columns >= ncols zero; out_scores the raw sums; out_lengths.
__global__ __launch_bounds__(64) void beam_gather_kernel(SkfBeamState s, int table, int ncols, int T, float alpha,
                                                         long long* __restrict__ out_tokens, float* __restrict__ out_scores,
                                                         int* __restrict__ out_lengths) {
  __shared__ int s_src[SKF_BEAM_MAX];
  const int g = blockIdx.x, lane = threadIdx.x, W = s.W;
  float sc = -INFINITY, ns = -INFINITY;
  int len = 0;
  if (lane < W) {
    sc = s.scores[g * W + lane];
    len = s.lengths[g * W + lane];
    ns = alpha == 0.f ? sc : sc / powf((5.0f + (float)len) / 6.0f, alpha);
    if (!(ns == ns)) ns = -INFINITY;
  }
  int rank = 0;
  for (int j = 0; j < W; ++j) {
    const float on = __shfl(ns, j, 64);
    rank += (on > ns || (on == ns && j < lane)) ? 1 : 0;
  }
  if (lane < W) {
    s_src[rank] = lane;
    out_scores[g * W + rank] = sc;
    out_lengths[g * W + rank] = len;
  }
  __syncthreads();
  for (int rr = 0; rr < W; ++rr) {
    const int* ar = s.anc + ((size_t)table * s.B + g * W + s_src[rr]) * s.anc_ld;
    long long* dst = out_tokens + (size_t)(g * W + rr) * T;
    for (int j = lane; j < T; j += 64) {
      long long v = 0;
      if (j < ncols) {
        int a = ar[j];
        a = a < 0 ? 0 : (a >= s.B ? s.B - 1 : a);
        v = s.tokens[(size_t)a * s.Ti + j];
      }
      dst[j] = v;
    }
  }
}

}  // namespace

int skf_beam_replicate(void* dst, const void* src, int n, int W, size_t cols, hipStream_t st) {
  hipLaunchKernelGGL(beam_replicate_kernel, dim3(skf_cdiv((long)cols, 256)), dim3(256), 0, st, (uint32_t*)dst, (const uint32_t*)src, n, W, cols);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

int skf_beam_init(const SkfBeamState& s, hipStream_t st) {
  hipLaunchKernelGGL(beam_init_kernel, dim3(1), dim3(256), 0, st, s);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

int skf_beam_advance_launch(const SkfBeamState& s, int step, int n_valid, long long eos, hipStream_t st) {
  SkfProfScope ps(st, "beam_advance", 0.0, 0.0);
  hipLaunchKernelGGL(beam_advance_kernel, dim3(s.n), dim3(64), 0, st, s, step, n_valid, eos);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

int skf_beam_gather(const SkfBeamState& s, int table, int ncols, int T, float alpha, long long* out_tokens, float* out_scores,
                    int* out_lengths, hipStream_t st) {
  hipLaunchKernelGGL(beam_gather_kernel, dim3(s.n), dim3(64), 0, st, s, table, ncols, T, alpha, out_tokens, out_scores, out_lengths);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

int skf_beam_check(const SkfBeam* b) {
  SKF_CHECK_ARG(b, "null SkfBeam");
  if (b->struct_size != sizeof(SkfBeam)) {
    skf_set_error("SkfBeam.struct_size is %u, this library's SkfBeam has %zu bytes (set struct_size = sizeof(SkfBeam))", b->struct_size,
                  sizeof(SkfBeam));
    return SKF_EINVAL;
  }
  SKF_CHECK_ARG(b->beam_width >= 1 && b->beam_width <= SKF_BEAM_MAX, "beam_width must be in [1, 8]");
  SKF_CHECK_ARG(b->length_alpha >= 0.f && b->length_alpha <= 3.0e38f, "length_alpha must be a finite number >= 0");
  return SKF_OK;
}

extern "C" int skf_beam_finish(const float* scores, const int* lengths, const int* ancestry, int ancestry_ld, const long long* tokens,
                               int tok_ld, int n, int beam_width, int ncols, int T, float length_alpha, long long* out_tokens,
                               float* out_scores, int* out_lengths, skf_stream_t stream) {
  SKF_CHECK_ARG(scores && lengths && ancestry && tokens && out_tokens && out_scores && out_lengths, "null operand");
  SKF_CHECK_ARG(beam_width >= 1 && beam_width <= SKF_BEAM_MAX, "beam_width must be in [1, 8]");
  SKF_CHECK_ARG(n >= 1 && (long long)n * beam_width <= 0x7fffffff / 8, "bad number of sketches");
  SKF_CHECK_ARG(ncols >= 1 && ncols <= T && ncols <= ancestry_ld && ncols <= tok_ld, "need 1 <= ncols <= min(T, ancestry_ld, tok_ld)");
  SKF_CHECK_ARG(length_alpha >= 0.f && length_alpha <= 3.0e38f, "length_alpha must be a finite number >= 0");
  SkfBeamState s{};
  s.n = n; s.W = beam_width; s.B = n * beam_width;
  s.scores = const_cast<float*>(scores); s.lengths = const_cast<int*>(lengths);
  s.anc = const_cast<int*>(ancestry); s.anc_ld = ancestry_ld; s.tokens = const_cast<long long*>(tokens); s.Ti = tok_ld;
  return skf_beam_gather(s, 0, ncols, T, length_alpha, out_tokens, out_scores, out_lengths, (hipStream_t)stream);
}

extern "C" int skf_beam_advance(const float* cand_logp, const int* cand_tok, int n, int beam_width, int step, long long eos,
                                float* scores, int* finished, int* lengths, int* ancestry, int ancestry_ld, long long* tokens,
                                int tok_ld, unsigned char* selfmask, int mask_ld, int* parent, skf_stream_t stream) {
  SKF_CHECK_ARG(cand_logp && cand_tok && scores && finished && lengths && ancestry && tokens && selfmask, "null operand");
  SKF_CHECK_ARG(beam_width >= 1 && beam_width <= SKF_BEAM_MAX, "beam_width must be in [1, 8]");
  SKF_CHECK_ARG(n >= 1 && (long long)n * beam_width <= 0x7fffffff / 8, "bad number of sketches");
  SKF_CHECK_ARG(step >= 0 && step + 1 < ancestry_ld && step + 1 < tok_ld && step + 1 < mask_ld, "position step + 1 must lie inside every row");
  SkfBeamState s{};
  s.n = n; s.W = beam_width; s.B = n * beam_width;
  s.cand_lp = const_cast<float*>(cand_logp); s.cand_tok = const_cast<int*>(cand_tok);
  s.scores = scores; s.finished = finished; s.lengths = lengths; s.anc = ancestry; s.anc_ld = ancestry_ld;
  s.tokens = tokens; s.Ti = tok_ld; s.selfmask = selfmask; s.mask_ld = mask_ld; s.parent = parent;
  return skf_beam_advance_launch(s, step, n, eos, (hipStream_t)stream);
}
