// One kernel per emitted position of the KV-cached greedy reconstruction (models/sketchformer.py:255-311
// predict_from_embedding; decoder layer = builders/layers/transformer.py:245-262, 325-344).
//
// The samples of a batch never interact during decoding, so one workgroup owns one sample and walks the whole step:
//   x = embed(token_i) * sqrt(d) + pos[i]
//   per layer: [q|k|v] = x Wqkv ; k|v appended to the cache ; attention of q over keys 0..i (target padding mask) ;
//              o-projection ; LN ; q2 = . Wq ; attention over the cached K|V of pre_decoder ; o-projection ; LN ; FFN ; LN
//   logits -> argmax (first index on ties), or a sampled token (skf_sample.h) / stroke-5 row -> appended ; EOS bookkeeping
// The round-1 path issued this as 51 dependent launches of ~7 us each (0.35 ms per position, all latency); here the
// activations of the position never leave LDS, and what the kernel waits for is the weight stream: every workgroup reads
// the decoder's weights (0.9 MB per layer at d = 128) from the L2 once per position - 16-byte loads, 16 in flight per thread
// (measured with per-phase clock stamps, cfg-2 dimensions, position 199: the six GEMVs of a layer 18 us = 25-30 B/cycle/CU,
// the two attentions 8 + 6 us (four dependent K / V round trips each), three LayerNorms 3 us, logits 6 us; 151 us in all).
// Each Dense is a GEMV: thread = 4 output columns x one slice of the contraction, partial sums folded through LDS in a
// fixed order (deterministic).
// The last workgroup to finish a position (ticket counter) does the cross-sample part: "all n_valid samples have emitted
// an EOS" -> done_step, and advances the device-side step index, so a position is ONE launch (captured once, replayed).
// Sketch completion (include/skf.h: prefix-forced decoding): where a prefix gives the position's token, the kernel emits it without
// computing logits; decode_prefill_kernel below produces the K | V cache rows of all such positions at once, layer by layer, from
// the device functions this kernel is made of, and a forced row then skips its layers as well.
#include "skf_common.h"
#include "skf_decode_fused.h"
#include "skf_sample.h"

namespace {

constexpr int NT = 512;   // threads per workgroup (8 waves)
static_assert(NT == SKF_SAMPLE_NT && 4 * NT >= SKF_SAMPLE_SCRATCH_FLOATS, "skf_sample_row runs on this workgroup, in the `part` area");
constexpr int UN = 16;   // weight rows requested per thread before the first is used

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
  v = wave_sum(v);
  __syncthreads();                       // red is reused from the previous reduction
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) t += red[w];
  return t;
}

// y[n] = act(bias[n] + sum_k x[k] W[k * ldw + n]), n < N.  x, y, part in LDS (y != x).  Ends with a barrier.
template <int VEC>
__device__ __forceinline__ void gemv(const float* __restrict__ W, int ldw, const float* __restrict__ bias, const float* x, float* y, int N,
                     int K, int act, float* part, int tid) {
  const int ncg = (N + VEC - 1) / VEC;
  int ks = 1;
  while (ks * 2 * ncg <= NT && K / (ks * 2) >= UN) ks *= 2;
  const int gp = ncg < NT / ks ? ncg : NT / ks;        // column groups per pass
  const int kch = (K + ks - 1) / ks;
  const int ksl = tid / gp, cgi = tid - ksl * gp;
  for (int base = 0; base < ncg; base += gp) {
    const int cg = base + cgi;
    if (ksl < ks && cg < ncg) {
      const int k0 = ksl * kch, k1 = k0 + kch < K ? k0 + kch : K;
      float acc[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
      const float* wp = W + (size_t)k0 * ldw + cg * VEC;
      int k = k0;
      for (; k + UN <= k1; k += UN) {
        if constexpr (VEC == 4) {
          f32x4 w[UN];
#pragma unroll
          for (int u = 0; u < UN; ++u) w[u] = *reinterpret_cast<const f32x4*>(wp + (size_t)u * ldw);
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const float xv = x[k + u];
            acc[0] += xv * w[u][0]; acc[1] += xv * w[u][1]; acc[2] += xv * w[u][2]; acc[3] += xv * w[u][3];
          }
        } else {
          float w[UN];
#pragma unroll
          for (int u = 0; u < UN; ++u) w[u] = wp[(size_t)u * ldw];
#pragma unroll
          for (int u = 0; u < UN; ++u) acc[0] += x[k + u] * w[u];
        }
        wp += (size_t)UN * ldw;
      }
      for (; k < k1; ++k) {
        const float xv = x[k];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += xv * wp[e];
        wp += ldw;
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) part[(ksl * gp + cgi) * VEC + e] = acc[e];
    }
    __syncthreads();
    for (int idx = tid; idx < gp * VEC; idx += NT) {
      const int n = base * VEC + idx;
      if (n < N) {
        float s = bias ? bias[n] : 0.f;
        for (int q = 0; q < ks; ++q) s += part[q * gp * VEC + idx];
        if (act == 1) s = fmaxf(s, 0.f);
        y[n] = s;
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void dense(const SkfDecDense& w, const float* x, float* y, int act, float* part, int tid) {
  if (w.vec4) gemv<4>(w.w, w.ld, w.b, x, y, w.out, w.in, act, part, tid);
  else gemv<1>(w.w, w.ld, w.b, x, y, w.out, w.in, act, part, tid);
}

// out = LayerNorm(a + r) (eps 1e-6, biased variance; builders/layers/transformer.py:217-222).  d <= NT.  Ends with a barrier.
__device__ __forceinline__ void add_ln(const float* a, const float* r, const float* __restrict__ g, const float* __restrict__ bt, float* out, int d,
                       float* red, int tid) {
  const float z = tid < d ? a[tid] + r[tid] : 0.f;
  const float mean = block_sum(z, red, tid) / (float)d;
  const float c = tid < d ? z - mean : 0.f;
  const float rstd = rsqrtf(block_sum(c * c, red, tid) / (float)d + 1e-6f);
  if (tid < d) out[tid] = c * rstd * g[tid] + bt[tid];
  __syncthreads();
}

// scaled_dot_product_attention (builders/utils.py:71-105) for one query row over the rows j < Lk of a (Lk, ld_kv) K / V image
// of the sample.  A thread owns one 16-byte column group c4 of the d columns and every (NT / (d/4))-th key, so a wave
// instruction reads whole contiguous rows (a lane per key would touch 64 cache lines per instruction: measured 10 of the
// 11 us of this function).  Three phases through LDS: scores[h][j] (dot product folded over the DH/4 adjacent lanes of a
// head), softmax per head (wave = head), weighted sum of V (partials per key slice, folded in a fixed order).
// aw non-null: head h's probabilities also go to aw[h * aw_hs + j] (lanes over keys: contiguous stores), zeros from Lk to aw_len.
// INDIRECT (beam search): key j of the hypothesis lives in another row's slot - Kb, Vb and mask are the bases of slot 0, and
// koff[j] / moff[j] (LDS, 32-bit, made once per position from the ancestry row) are the offsets of its K | V row in floats and of
// its mask byte; the direct form is the code it was before the beam instantiation existed.
template <int DH, bool INDIRECT = false>
__device__ __forceinline__ void attend(const float* q_lds, const float* __restrict__ Kb, const float* __restrict__ Vb, int ld_kv, int Lk,
                       const unsigned char* __restrict__ mask, int limit, int d, int H, float* sc, int LkP, float* part,
                       float* o_lds, int tid, float* __restrict__ aw, size_t aw_hs, int aw_len, const unsigned* koff = nullptr,
                       const unsigned* moff = nullptr) {
  const int nc4 = d >> 2, jl = tid / nc4, c4 = tid - jl * nc4, JP = NT / nc4;
  const int h = (4 * c4) / DH;
  const f32x4 q4 = *reinterpret_cast<const f32x4*>(q_lds + 4 * c4);
  const float scale_div = sqrtf((float)DH);
  // All rows of a thread are requested before the first is used (a row-at-a-time loop costs one L2 / HBM round trip per
  // row), V together with K: up to NR rows of each stay in registers; longer key ranges go round the loop again.
  constexpr int NR = 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bool one_pass = Lk <= NR * JP;
  f32x4 kv[NR], vv[NR];
#define SKF_LOAD_ROWS(base, r, j0)                                                                              \
  _Pragma("unroll") for (int u = 0; u < NR; ++u) {                                                              \
    const int j = (j0) + u * JP;                                                                                \
    if constexpr (INDIRECT) {                                                                                   \
      const int jc = j < Lk ? j : Lk - 1;                                                                       \
      r[u] = *reinterpret_cast<const f32x4*>((base) + koff[jc] + 4 * c4);                                      \
    } else {                                                                                                    \
      r[u] = *reinterpret_cast<const f32x4*>((base) + (size_t)(j < Lk ? j : Lk - 1) * ld_kv + 4 * c4);         \
    }                                                                                                           \
  }
#define SKF_SCORES(j0)                                                                                          \
  _Pragma("unroll") for (int u = 0; u < NR; ++u) {                                                              \
    const int j = (j0) + u * JP;                                                                                \
    float dot = q4[0] * kv[u][0] + q4[1] * kv[u][1] + q4[2] * kv[u][2] + q4[3] * kv[u][3];                      \
    _Pragma("unroll") for (int o = 1; o < DH / 4; o <<= 1) dot += __shfl_xor(dot, o, 64);                       \
    if (j < Lk && (c4 & (DH / 4 - 1)) == 0) {                                                                   \
      bool masked;                                                                                              \
      if constexpr (INDIRECT) masked = mask[moff[j]] || j >= limit;                                             \
      else masked = (mask && mask[j]) || j >= limit;                                                            \
      sc[h * LkP + j] = dot / scale_div + (masked ? -1e9f : 0.f);                                               \
    }                                                                                                           \
  }
#define SKF_WEIGHTED(j0)                                                                                        \
  _Pragma("unroll") for (int u = 0; u < NR; ++u) {                                                              \
    const int j = (j0) + u * JP;                                                                                \
    const float pj = j < Lk ? sc[h * LkP + j] : 0.f;                                                            \
    acc[0] += pj * vv[u][0]; acc[1] += pj * vv[u][1]; acc[2] += pj * vv[u][2]; acc[3] += pj * vv[u][3];         \
  }
  SKF_LOAD_ROWS(Kb, kv, jl)
  if (one_pass) { SKF_LOAD_ROWS(Vb, vv, jl) }
  SKF_SCORES(jl)
  for (int j0 = jl + NR * JP; j0 < Lk; j0 += NR * JP) { SKF_LOAD_ROWS(Kb, kv, j0) SKF_SCORES(j0) }
  __syncthreads();
  {
    const int lane = tid & 63, wave = tid >> 6;
    for (int hh = wave; hh < H; hh += NT / 64) {
      float* row = sc + hh * LkP;
      float mx = -INFINITY;
      for (int j = lane; j < Lk; j += 64) mx = fmaxf(mx, row[j]);
      mx = wave_max(mx);
      float se = 0.f;
      for (int j = lane; j < Lk; j += 64) { const float e = __expf(row[j] - mx); row[j] = e; se += e; }
      se = wave_sum(se);
      const float rinv = 1.0f / se;
      if (aw) {                  // uniform; a constant null in the weights-off instantiation (the branch folds away)
        float* dst = aw + hh * aw_hs;
        for (int j = lane; j < Lk; j += 64) { const float pj = row[j] * rinv; row[j] = pj; dst[j] = pj; }
        for (int j = Lk + lane; j < aw_len; j += 64) dst[j] = 0.f;
      } else {
        for (int j = lane; j < Lk; j += 64) row[j] *= rinv;
      }
    }
  }
  __syncthreads();
  if (one_pass) { SKF_WEIGHTED(jl) }
  else for (int j0 = jl; j0 < Lk; j0 += NR * JP) { SKF_LOAD_ROWS(Vb, vv, j0) SKF_WEIGHTED(j0) }
#undef SKF_LOAD_ROWS
#undef SKF_SCORES
#undef SKF_WEIGHTED
  *reinterpret_cast<f32x4*>(part + jl * d + 4 * c4) = acc;
  __syncthreads();
  for (int c = tid; c < d; c += NT) {
    float t = 0.f;
    for (int q = 0; q < JP; ++q) t += part[q * d + c];
    o_lds[c] = t;
  }
  __syncthreads();
}

// Beam search: the row's log-softmax in place (one max, one sum of expf, both folded in a fixed order) and its W best (log p, token)
// pairs, log p descending, then token ascending.  NaN ranks as -inf.  W rounds of a workgroup arg-max over the entries behind the
// previous pick in that order (W <= 8, W <= V).  hs[0..V): the logits, complete and visible; scratch: 32 floats.
__device__ __forceinline__ void beam_candidates(float* hs, int V, int W, float* __restrict__ cand_lp, int* __restrict__ cand_tok,
                                                float* scratch, int tid) {
  float* wv = scratch;                                  // [8] per-wave value
  int* wj = reinterpret_cast<int*>(scratch + 8);        // [8] per-wave index
  const int lane = tid & 63, wave = tid >> 6;
  float m = -INFINITY;
  for (int j = tid; j < V; j += NT) {
    float v = hs[j];
    if (!(v == v)) { v = -INFINITY; hs[j] = v; }
    m = fmaxf(m, v);
  }
  m = wave_max(m);
  if (lane == 0) wv[wave] = m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) m = fmaxf(m, wv[w]);
  float se = 0.f;
  for (int j = tid; j < V; j += NT) se += expf(hs[j] - m);
  se = wave_sum(se);
  __syncthreads();
  if (lane == 0) wv[wave] = se;
  __syncthreads();
  se = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) se += wv[w];
  const float lse = m + logf(se);
  for (int j = tid; j < V; j += NT) {
    float lp = hs[j] - lse;
    if (!(lp == lp)) lp = -INFINITY;                    // a row without a finite maximum has no distribution
    hs[j] = lp;
  }
  float pv = INFINITY;
  int pj = -1;
  for (int k = 0; k < W; ++k) {
    __syncthreads();                                    // hs complete; wv / wj free again
    float bv = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = tid; j < V; j += NT) {
      const float v = hs[j];
      const bool behind = v < pv || (v == pv && j > pj);
      if (behind && (v > bv || (v == bv && j < bj))) { bv = v; bj = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64); const int oj = __shfl_xor(bj, o, 64);
      if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
    }
    if (lane == 0) { wv[wave] = bv; wj[wave] = bj; }
    __syncthreads();
    bv = wv[0]; bj = wj[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w)
      if (wv[w] > bv || (wv[w] == bv && wj[w] < bj)) { bv = wv[w]; bj = wj[w]; }
    if (tid == 0) { cand_lp[k] = bv; cand_tok[k] = bj < V ? bj : 0; }
    pv = bv; pj = bj;
  }
}

// The workgroup's LDS areas, the same in the position kernel and in the prefill kernel.
struct DecLds {
  float* xs;      // [d]  layer input
  float* o1;      // [d]  after LN1
  float* o2;      // [d]  after LN2
  float* ys;      // [d]  Dense output awaiting its residual
  float* os;      // [d]  attention output
  float* qkv;     // [3d]
  float* hs;      // [max(F, Vout)] FFN hidden / logits
  float* part;    // [4 NT] GEMV partial sums
  float* red;     // [16]
  float* sc;      // [H][LkP] attention scores / probabilities
};

__device__ __forceinline__ DecLds dec_lds(float* lds, int d, int hs_len) {
  DecLds a;
  a.xs = lds; a.o1 = a.xs + d; a.o2 = a.o1 + d; a.ys = a.o2 + d; a.os = a.ys + d; a.qkv = a.os + d;
  a.hs = a.qkv + 3 * d; a.part = a.hs + hs_len; a.red = a.part + 4 * NT; a.sc = a.red + 16;
  return a;
}

// decoder input of one position (builders/layers/transformer.py:325-334, dropout off); token mode.  Ends with a barrier.
__device__ __forceinline__ void embed_token(const SkfDecodeFused& p, long long tk, int pos_i, float* xs, int d, int tid) {
  if (tid < d) {
    if (tk < 0 || tk >= p.vocab) tk = 0;
    const float v = p.emb_table[(size_t)tk * d + tid];
    xs[tid] = v * sqrtf((float)d) + p.pos[(size_t)pos_i * d + tid];
  }
  __syncthreads();
}

// The two halves of a decoder layer on either side of its self-attention, shared by the position kernel and the prefill kernel.
// layer_qkv: [q|k|v] = xs Wqkv into a.qkv, k|v appended to the cache as `cache_row`.  Ends with a barrier (the appended row is read
// back by the attention: workgroup-scope visibility of the global stores).
__device__ __forceinline__ void layer_qkv(const SkfDecLayer& w, const DecLds& a, float* __restrict__ cache_row, int d, int tid) {
  dense(w.qkv, a.xs, a.qkv, 0, a.part, tid);
  for (int c = tid; c < 2 * d; c += NT) cache_row[c] = a.qkv[d + c];
  __syncthreads();
}

// layer_rest: from the self-attention output a.os to the layer's output in a.xs: o-projection ; LN ; cross attention over kv2 (keys
// >= limit masked) ; o-projection ; LN ; FFN ; LN.  aw2: where the cross-attention weights go, or null.
template <int DH>
__device__ __forceinline__ void layer_rest(const SkfDecLayer& w, const DecLds& a, const float* __restrict__ kv2, int limit, int d, int H,
                                           int Le, int LkP, int tid, float* __restrict__ aw2, size_t aw_hs) {
  dense(w.o, a.os, a.ys, 0, a.part, tid);
  add_ln(a.xs, a.ys, w.ln1_g, w.ln1_b, a.o1, d, a.red, tid);
  dense(w.q2, a.o1, a.qkv, 0, a.part, tid);
  attend<DH>(a.qkv, kv2, kv2 + d, 2 * d, Le, nullptr, limit, d, H, a.sc, LkP, a.part, a.os, tid, aw2, aw_hs, Le);
  dense(w.o2, a.os, a.ys, 0, a.part, tid);
  add_ln(a.o1, a.ys, w.ln2_g, w.ln2_b, a.o2, d, a.red, tid);
  dense(w.f1, a.o2, a.hs, 1, a.part, tid);
  dense(w.f2, a.hs, a.ys, 0, a.part, tid);
  add_ln(a.o2, a.ys, w.ln3_g, w.ln3_b, a.xs, d, a.red, tid);
}

// cross attention: keys >= limit are masked (models/sketchformer.py:172,279-283)
__device__ __forceinline__ int cross_limit(const SkfDecodeFused& p, int b, int step) {
  int limit = 0x7fffffff;
  if (!p.blind) { limit = p.limit ? p.limit[b] : -1; if (limit < 0) limit = step + 1; }
  return limit;
}

// The token a prefix forces on row b at position `step` (include/skf.h: prefix-forced decoding), or -1 where the position is free.
// A token outside [0, vocab) counts as PAD, as in the embedding lookup.
__device__ __forceinline__ int forced_token(const SkfDecodeFused& p, int b, int step) {
  if (!p.prefix || step >= p.prefix_len[b]) return -1;
  const long long tk = p.prefix[(size_t)b * p.prefix_ld + step];
  return tk < 0 || tk >= p.vocab ? 0 : (int)tk;
}

// AW: the instantiation that writes the attention weights; the other one is the decoder without that output.
// SAMPLE: the token is drawn (temperature / top-k / nucleus, skf_sample.h) instead of maximised; what follows the choice is shared.
// BEAM: the history is read through the ancestry table and the kernel ends with the row's W best candidates (skf_beam.hip).
template <int DH, bool AW, bool SAMPLE, bool BEAM = false>
__global__ __launch_bounds__(NT) void decode_position_kernel(SkfDecodeFused p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int d = p.d;
  const DecLds a = dec_lds(lds, d, p.hs_len);
  float *const xs = a.xs, *const hs = a.hs, *const part = a.part, *const sc = a.sc;
  const int LkP = p.Le + 1;
  const int step = *p.step_dev;
  // BEAM: where positions 0..step of the hypothesis live, as offsets from slot 0: [Le + 1] K | V rows (floats), [Le + 1] mask bytes
  unsigned* koff = reinterpret_cast<unsigned*>(sc + p.H * LkP);
  unsigned* moff = koff + LkP;
  if constexpr (BEAM) {
    const int* ar = p.anc + ((size_t)(step & 1) * p.B + b) * LkP;
    for (int j = tid; j <= step; j += NT) {
      int a = ar[j];
      a = j == step ? b : (a < 0 ? 0 : (a >= p.B ? p.B - 1 : a));           // the newest row is the workgroup's own
      koff[j] = ((unsigned)a * (unsigned)p.Le + (unsigned)j) * (unsigned)(2 * d);      // (the launcher checks B Le 2d < 2^32)
      moff[j] = (unsigned)a * (unsigned)p.mask_ld + (unsigned)j;
    }
  }
  const int n_valid = (int)p.dyn[0];
  const long long eos = p.dyn[1];
  // prefix-forced decoding (include/skf.h): the position's token is given, so it needs no logits; after a prefill (skf_decode_prefill_launch)
  // its K | V rows exist as well and the layers are skipped too.  Workgroup-uniform.  No prefix: the code below is what it was.
  const int ftok = AW ? -1 : forced_token(p, b, step);
  const bool forced = ftok >= 0;
  if (BEAM || !forced || !p.prefilled) {
    // decoder input of the position (builders/layers/transformer.py:325-334, dropout off)
    if (tid < d) {
      float v;
      if (p.tokens) {
        long long tk = p.tokens[(size_t)b * p.Ti + step];
        if (tk < 0 || tk >= p.vocab) tk = 0;
        v = p.emb_table[(size_t)tk * d + tid];
      } else {
        const float* x = p.cont + ((size_t)b * p.Ti + step) * 5;
        const float* W = p.embd_w;
        v = x[0] * W[tid] + x[1] * W[d + tid] + x[2] * W[2 * d + tid] + x[3] * W[3 * d + tid] + x[4] * W[4 * d + tid] + p.embd_b[tid];
      }
      xs[tid] = v * sqrtf((float)d) + p.pos[(size_t)step * d + tid];
    }
    __syncthreads();

    const int limit = cross_limit(p, b, step);
    const unsigned char* smask = p.selfmask + (size_t)b * p.mask_ld;
    // attention weights of the position: row `step` of (2N, B, H, attn_rows, Le); block k of layer l at + (2l + k) * blk
    const size_t aw_hs = (size_t)p.attn_rows * p.Le, aw_blk = (size_t)p.B * p.H * aw_hs;
    float* aw = AW && step < p.attn_rows ? p.attn + ((size_t)b * p.H * p.attn_rows + step) * p.Le : nullptr;

    for (int l = 0; l < p.N; ++l) {
      const SkfDecLayer& w = p.layer[l];
      float* cache = w.cache + (size_t)b * p.Le * 2 * d;             // (Le, 2d): K | V of the positions so far
      layer_qkv(w, a, cache + (size_t)step * 2 * d, d, tid);
      if constexpr (BEAM)
        attend<DH, true>(a.qkv, w.cache, w.cache + d, 2 * d, step + 1, p.selfmask, 0x7fffffff, d, p.H, a.sc, LkP, a.part, a.os, tid, nullptr, 0, 0,
                         koff, moff);
      else
        attend<DH>(a.qkv, cache, cache + d, 2 * d, step + 1, smask, 0x7fffffff, d, p.H, a.sc, LkP, a.part, a.os, tid,
                   aw ? aw + (size_t)(2 * l) * aw_blk : nullptr, aw_hs, p.Le);
      layer_rest<DH>(w, a, w.kv2 + (size_t)b * p.Le * 2 * d, limit, d, p.H, p.Le, LkP, tid,
                     aw ? aw + (size_t)(2 * l + 1) * aw_blk : nullptr, aw_hs);
    }
  }
  if (!forced) dense(p.out, xs, hs, 0, part, tid);          // logits of the position (F >= Vout is not assumed: hs holds max(F, Vout))

  if constexpr (BEAM) {
    if (forced) {      // a live beam offers exactly one candidate, (0, the prefix token); beam_advance_kernel is what it was
      if (tid < p.beam) {
        p.cand_lp[(size_t)b * p.beam + tid] = tid == 0 ? 0.f : -INFINITY;
        p.cand_tok[(size_t)b * p.beam + tid] = tid == 0 ? ftok : 0;
      }
      return;
    }
    beam_candidates(hs, p.Vout, p.beam, p.cand_lp + (size_t)b * p.beam, p.cand_tok + (size_t)b * p.beam, part, tid);
    return;
  }
  __shared__ float s_mx[NT / 64];
  __shared__ int s_am[NT / 64];
  if (p.tokens) {
    // models/sketchformer.py:285-301: next = argmax (first index on ties, tf.argmax); PAD masks the key in later steps;
    // EOS flags are sticky
    int am;
    if (forced) {
      am = ftok;
    } else if constexpr (SAMPLE) {
      am = skf_sample_row(hs, p.Vout, p.temperature, p.top_k, p.top_p,
                          skf_sample_bits24(p.seed, (uint32_t)p.stream_ids[b], (uint32_t)step), part, tid);
    } else {
      float mx = -INFINITY; am = 0x7fffffff;
      for (int j = tid; j < p.Vout; j += NT) {
        const float v = hs[j];
        if (v > mx) { mx = v; am = j; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64); const int oa = __shfl_xor(am, o, 64);
        if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
      }
      if ((tid & 63) == 0) { s_mx[tid >> 6] = mx; s_am[tid >> 6] = am; }
      __syncthreads();
      if (tid == 0) {
        for (int wv = 1; wv < NT / 64; ++wv)
          if (s_mx[wv] > mx || (s_mx[wv] == mx && s_am[wv] < am)) { mx = s_mx[wv]; am = s_am[wv]; }
      }
    }
    if (tid == 0) {
      p.tokens[(size_t)b * p.Ti + step + 1] = am;
      p.selfmask[(size_t)b * p.mask_ld + step + 1] = am == 0 ? 1 : 0;
      if ((long long)am == eos) p.eos_seen[b] = 1;
    }
  } else if (tid == 0) {
    // continuous: appended row = (x, y, softmax(pen logits)); mask byte = (row[4] == 1); "finished" = argmax(pen) == 2 (not sticky)
    const float* x = hs;
    const float m = fmaxf(x[2], fmaxf(x[3], x[4]));
    const float e0 = __expf(x[2] - m), e1 = __expf(x[3] - m), e2 = __expf(x[4] - m);
    const float r = 1.0f / (e0 + e1 + e2);
    float* o = p.cont + ((size_t)b * p.Ti + step + 1) * 5;
    const float q0 = e0 * r, q1 = e1 * r, q2 = e2 * r;
    o[0] = x[0]; o[1] = x[1]; o[2] = q0; o[3] = q1; o[4] = q2;
    p.selfmask[(size_t)b * p.mask_ld + step + 1] = (q2 == 1.0f) ? 1 : 0;
    const int am = (q0 >= q1 && q0 >= q2) ? 0 : (q1 >= q2 ? 1 : 2);
    p.eos_seen[b] = am == 2 ? 1 : 0;
  }
  // ---- cross-sample part, by whichever workgroup finishes the position last
  if (tid == 0) {
    __threadfence();
    const int t = atomicAdd(p.ticket, 1);
    if (t == p.B - 1) {
      __threadfence();
      int seen = 0;
      for (int i = 0; i < n_valid; ++i) seen += __hip_atomic_load(p.eos_seen + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seen >= n_valid && *p.done_step < 0) *p.done_step = step;
      *p.step_dev = step + 1;
      *p.ticket = 0;
    }
  }
}

// ---- prefill: the K | V cache rows of a known prefix, all positions at once (include/skf.h: prefix-forced decoding)
// The tokens of a prefix are known in advance, so its positions depend on each other only through the cache rows of the layer
// below.  Launch l (l = 0 .. N-1) runs one workgroup per (position s, row b) with s < len[b]:
//   launch 0:      x = embed(prefix column s) * sqrt(d) + pos[s] ; q|k|v of layer 0 ; cache row s of layer 0
//   launch l >= 1: the rest of layer l-1 (self-attention of q over cache rows 0..s, ..., LN3) ; q|k|v of layer l ; its cache row
// x and q of the position travel from launch l to launch l + 1 in the position's cache row of layer l + 1, which nobody reads before
// that launch has replaced them by the layer's k | v: a workgroup touches only its own row, and reads it before it writes it.
// Nothing follows the last layer's cache row: a forced position needs neither that layer's tail nor the logits.
// Every (b, s) calls the device functions the position kernel calls at step s, with the same arguments: the rows are bit-equal.
// Four waves per SIMD = two workgroups per CU: without the bound the allocator stops at 130 VGPRs, two above the 128 that allow it.
template <int DH>
__global__ __launch_bounds__(NT, 4) void decode_prefill_kernel(SkfDecodeFused p, int l) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
  if (s >= p.prefix_len[b] || s >= p.Le) return;
  const int d = p.d, LkP = p.Le + 1;
  const DecLds a = dec_lds(lds, d, p.hs_len);
  float* const row = p.layer[l].cache + ((size_t)b * p.Le + s) * 2 * d;       // x | q of the launch before, k | v from here on
  if (l == 0) {
    embed_token(p, p.tokens[(size_t)b * p.Ti + s], s, a.xs, d, tid);          // column s: the start symbol or prefix token s - 1
  } else {
    const SkfDecLayer& w = p.layer[l - 1];
    if (tid < d) { a.xs[tid] = row[tid]; a.qkv[tid] = row[d + tid]; }
    __syncthreads();
    const float* cache = w.cache + (size_t)b * p.Le * 2 * d;
    attend<DH>(a.qkv, cache, cache + d, 2 * d, s + 1, p.selfmask + (size_t)b * p.mask_ld, 0x7fffffff, d, p.H, a.sc, LkP, a.part, a.os, tid,
               nullptr, 0, p.Le);
    layer_rest<DH>(w, a, w.kv2 + (size_t)b * p.Le * 2 * d, cross_limit(p, b, s), d, p.H, p.Le, LkP, tid, nullptr, 0);
  }
  layer_qkv(p.layer[l], a, row, d, tid);
  if (l + 1 < p.N && tid < d) {
    float* next = p.layer[l + 1].cache + ((size_t)b * p.Le + s) * 2 * d;
    next[tid] = a.xs[tid]; next[d + tid] = a.qkv[tid];
  }
}

// What the positions a prefill skips would have left behind.  One workgroup.  Every row's prefix tokens and mask bytes go to their
// columns; with S0 = the shortest prefix of the B rows, the flags and done_step are those after positions 0 .. S0-1, and *step_dev = S0.
__global__ __launch_bounds__(256) void decode_prefill_init_kernel(SkfDecodeFused p) {
  __shared__ int s_min[256], s_last[256];
  const int tid = threadIdx.x;
  const int n_valid = (int)p.dyn[0];
  const long long eos = p.dyn[1];
  int mn = 0x7fffffff;
  for (int b = tid; b < p.B; b += 256) { const int n = p.prefix_len[b]; mn = n < mn ? n : mn; }
  s_min[tid] = mn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_min[tid] = s_min[tid + o] < s_min[tid] ? s_min[tid + o] : s_min[tid];
    __syncthreads();
  }
  int S0 = s_min[0];
  S0 = S0 < 0 ? 0 : (S0 > p.Le ? p.Le : S0);
  int last = -1;                // the latest first-EOS position among this thread's rows of the stop test; Le: a row without one
  for (int b = tid; b < p.B; b += 256) {
    int n = p.prefix_len[b];
    n = n > p.Le ? p.Le : n;
    int first = p.Le;
    for (int s = 0; s < n; ++s) {
      const int tk = forced_token(p, b, s);
      p.tokens[(size_t)b * p.Ti + s + 1] = tk;
      p.selfmask[(size_t)b * p.mask_ld + s + 1] = tk == 0 ? 1 : 0;
      if (s < S0 && first == p.Le && (long long)tk == eos) first = s;
    }
    if (first < p.Le) p.eos_seen[b] = 1;
    if (b < n_valid) last = first > last ? first : last;
  }
  s_last[tid] = last;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 256; ++k) last = s_last[k] > last ? s_last[k] : last;
    if (last >= 0 && last < p.Le) *p.done_step = last;
    *p.step_dev = S0;
  }
}

}  // namespace

size_t skf_decode_fused_lds_bytes(const SkfDecodeFused& p) {
  return (size_t)(8 * p.d + p.hs_len + 4 * NT + 16 + p.H * (p.Le + 1)) * sizeof(float);
}

int skf_decode_prefill_launch(const SkfDecodeFused& p, int max_len, hipStream_t st) {
  if (!p.prefix || !p.prefix_len || !p.tokens || p.beam || p.attn || max_len < 0 || max_len > p.Le) {
    skf_set_error("%s: the prefill needs token mode, a prefix, and no beams or attention output", __func__);
    return SKF_EINVAL;
  }
  {
    SkfProfScope ps(st, "decode_prefill_init", 0.0, 0.0);
    hipLaunchKernelGGL(decode_prefill_init_kernel, dim3(1), dim3(256), 0, st, p);
    SKF_LAUNCH_CHECK();
  }
  if (max_len == 0) return SKF_OK;
  const int dh = p.d / p.H;
  const size_t smem = skf_decode_fused_lds_bytes(p);
  SkfProfScope ps(st, "decode_prefill", 0.0, 0.0);
#define SKF_DP(DHV)                                                                                                  \
  {                                                                                                                  \
    SKF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_prefill_kernel<DHV>),                            \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));                              \
    for (int l = 0; l < p.N; ++l)                                                                                    \
      hipLaunchKernelGGL((decode_prefill_kernel<DHV>), dim3(max_len, p.B), dim3(NT), smem, st, p, l);                \
  }
  if (dh == 16) SKF_DP(16) else if (dh == 32) SKF_DP(32) else SKF_DP(64)
#undef SKF_DP
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

bool skf_decode_fused_supported(int d, int H, int F, int Le, int N, int Vout) {
  const int dh = H > 0 ? d / H : 0;
  return d <= NT && (d & 3) == 0 && NT % (d / 4) == 0 && (dh == 16 || dh == 32 || dh == 64) && N <= SKF_DEC_MAX_LAYERS && F > 0 && Vout > 0 &&
         (size_t)(8 * d + (F > Vout ? F : Vout) + 4 * NT + 16 + H * (Le + 1)) * sizeof(float) <= 159 * 1024;
}

bool skf_decode_beam_supported(int d, int H, int F, int Le, int N, int Vout) {
  return skf_decode_fused_supported(d, H, F, Le, N, Vout) &&
         (size_t)(8 * d + (F > Vout ? F : Vout) + 4 * NT + 16 + (H + 2) * (Le + 1)) * sizeof(float) <= 159 * 1024;
}

int skf_decode_fused_launch(const SkfDecodeFused& p, hipStream_t st) {
  const int dh = p.d / p.H;
  if (p.beam) {
    if (p.attn || p.sample || !p.tokens || !p.anc || !p.cand_lp || !p.cand_tok || p.beam > SKF_BEAM_MAX || p.beam > p.Vout ||
        p.beam_rows < p.beam || p.beam_rows > p.B || (unsigned long long)p.B * p.Le * 2 * p.d >= (1ull << 32) || p.mask_ld != p.Le + 1) {
      skf_set_error("%s: beam search needs token mode, its ancestry and candidate areas, 1 <= W <= min(8, vocab) and no attention output", __func__);
      return SKF_EINVAL;
    }
    const size_t smem = skf_decode_fused_lds_bytes(p) + (size_t)2 * (p.Le + 1) * sizeof(int);
    SkfProfScope ps(st, "decode_position_beam", 0.0, 0.0);
#define SKF_DB(DHV)                                                                                                  \
  {                                                                                                                  \
    SKF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_position_kernel<DHV, false, false, true>),       \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));                              \
    hipLaunchKernelGGL((decode_position_kernel<DHV, false, false, true>), dim3(p.beam_rows), dim3(NT), smem, st, p); \
  }
    if (dh == 16) SKF_DB(16) else if (dh == 32) SKF_DB(32) else SKF_DB(64)
#undef SKF_DB
    SKF_LAUNCH_CHECK();
    return SKF_OK;
  }
  const size_t smem = skf_decode_fused_lds_bytes(p);
  SkfProfScope ps(st, "decode_position", 0.0, 0.0);
#define SKF_DF(DHV, AWV, SMV)                                                                                        \
  {                                                                                                                  \
    SKF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_position_kernel<DHV, AWV, SMV>),                 \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024)); /* per launch: per-device attribute */ \
    hipLaunchKernelGGL((decode_position_kernel<DHV, AWV, SMV>), dim3(p.B), dim3(NT), smem, st, p);                   \
  }
  if (p.sample) {                  // (no attention-weight output with sampling: nothing asks for it)
    if (p.attn || !p.tokens || !p.stream_ids) { skf_set_error("%s: sampling needs token mode, stream ids and no attention output", __func__); return SKF_EINVAL; }
    if (dh == 16) SKF_DF(16, false, true) else if (dh == 32) SKF_DF(32, false, true) else SKF_DF(64, false, true)
  } else if (p.attn) {
    if (dh == 16) SKF_DF(16, true, false) else if (dh == 32) SKF_DF(32, true, false) else SKF_DF(64, true, false)
  } else {
    if (dh == 16) SKF_DF(16, false, false) else if (dh == 32) SKF_DF(32, false, false) else SKF_DF(64, false, false)
  }
#undef SKF_DF
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
