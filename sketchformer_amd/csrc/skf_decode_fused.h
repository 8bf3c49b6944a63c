// Argument block of the one-launch-per-position greedy decode (skf_decode_fused.hip) and the attention launcher of the
// layer-by-layer decode (skf_decode.hip); internal to libskf.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/skf.h"

constexpr int SKF_DEC_MAX_LAYERS = 8;

struct SkfDecDense { const float* w; const float* b; int in, out, ld, vec4; };   // W[in][out], row stride ld; vec4: 16-byte column groups allowed

struct SkfDecLayer {
  SkfDecDense qkv, o, q2, o2, f1, f2;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
  float* cache;           // (B, Le, 2d): self-attention K | V rows of the positions decoded so far
  const float* kv2;       // (B, Le, 2d): cross-attention K | V of pre_decoder
};

struct SkfDecodeFused {
  int B, Le, d, H, F, N, Vout, vocab, blind, hs_len;
  SkfDecLayer layer[SKF_DEC_MAX_LAYERS];
  SkfDecDense out;
  const float* emb_table; const float* embd_w; const float* embd_b; const float* pos;
  long long* tokens; float* cont; int Ti;         // running output image (B, Ti[, 5]); exactly one of tokens / cont
  unsigned char* selfmask; int mask_ld;
  int* eos_seen; int* done_step; int* step_dev; int* ticket;
  const long long* dyn;                           // [0] n_valid, [1] eos
  const int* limit;                               // per-sample cross-attention key limit (non-blind) or null
  float* attn; int attn_rows;                     // null, or (2N, B, H, attn_rows, Le) softmax rows: [2l] self, [2l+1] cross; row = step
  // sample != 0 (token mode): the token is drawn by the selection rule of include/skf.h with u = uniform(seed, stream_ids[b], step)
  int sample; float temperature; int top_k; float top_p; unsigned seed;
  const int* stream_ids;                          // (B) device
  // beam != 0 (token mode, skf_model_beam_decode): beam width W; the first beam_rows = n W rows are at work (the grid).  The
  // workgroup reads the history of its hypothesis through row b of ancestry table step & 1 and writes its W best (log p, token)
  // pairs; tokens, flags, ticket and step index belong to beam_advance_kernel (skf_beam.hip)
  int beam, beam_rows;
  const int* anc;                                 // (2, B, Le + 1)
  float* cand_lp; int* cand_tok;                  // (B, W), log p descending, then token ascending
  // prefix != null (token mode, no attention output; include/skf.h: prefix-forced decoding): position s of row b is forced iff
  // s < prefix_len[b]; it emits prefix[b][s] and computes no logits (BEAM: its one candidate is (0, that token)).  prefilled: the
  // cache rows of every forced position exist already (skf_decode_prefill_launch), so a forced row skips the layers as well.
  const long long* prefix; int prefix_ld;         // (B, prefix_ld) device
  const int* prefix_len;                          // (B) device
  int prefilled;
};

bool skf_decode_fused_supported(int d, int H, int F, int Le, int N, int Vout);
// the same for the beam instantiation, whose workgroup also keeps the offsets of its history (2 (Le + 1) ints) in LDS
bool skf_decode_beam_supported(int d, int H, int F, int Le, int N, int Vout);
int skf_decode_fused_launch(const SkfDecodeFused& p, hipStream_t st);
// The cache rows 0 .. prefix_len[b]-1 of every layer and row in N launches over (max_len, B) workgroups, behind one small launch that
// writes the prefix columns, flags and done_step the skipped positions would have left, and *step_dev = min_b prefix_len[b].
// max_len >= every prefix_len[b] (the grid); the tokens' column 0 (skf_decode_init), dyn and the cross K|V must be in place.
int skf_decode_prefill_launch(const SkfDecodeFused& p, int max_len, hipStream_t st);

// SkfSampling as the public entries take it: struct_size, temperature > 0, top_k >= 0, 0 < top_p <= 1 (SKF_EINVAL otherwise)
int skf_sampling_check(const SkfSampling* s);

// skf_attention_decode plus an optional copy of the softmax rows: attn (B, H, attn_rows, attn_ld), row *step_dev of every
// (sample, head) = the Lk probabilities, then zeros up to attn_ld (attn non-null needs step_dev).
int skf_attention_decode_w(const float* Q, int ldq, const float* K, const float* V, int ld_kv, long long kv_batch_stride,
                           const unsigned char* key_mask, int key_mask_ld, const int* key_limit, int key_limit_all, int B, int H,
                           int Lk, int dh, float* O, int ldo, const int* step_dev, const float* K_new, const float* V_new, int ld_new,
                           int limit_from_step, float* attn, int attn_rows, int attn_ld, hipStream_t stream);

// ---- beam search (skf_beam.hip).  State of n sketches x W beams in rows g W + k of B-row areas.
struct SkfBeamState {
  int n, W, B;
  float* cand_lp; int* cand_tok;                  // (B, W): what the position kernel offers
  float* scores; int* finished; int* lengths;     // (B): fp32 sum of log p, sticky EOS flag, position of the EOS (else positions emitted)
  int* anc; int anc_ld;                           // (2, B, anc_ld) ancestry tables
  long long* tokens; int Ti; unsigned char* selfmask; int mask_ld;
  int* parent;                                    // optional (B): the parent beam of every survivor (stand-alone entry)
  int* done_step; int* step_dev; int* ticket; const long long* dyn;      // null in the stand-alone entry: step, n_valid, eos are arguments
};
int skf_beam_check(const SkfBeam* b);
int skf_beam_replicate(void* dst, const void* src, int n, int W, size_t cols_4byte, hipStream_t st);
int skf_beam_init(const SkfBeamState& s, hipStream_t st);
int skf_beam_advance_launch(const SkfBeamState& s, int step, int n_valid, long long eos, hipStream_t st);
int skf_beam_gather(const SkfBeamState& s, int table, int ncols, int T, float alpha, long long* out_tokens, float* out_scores,
                    int* out_lengths, hipStream_t st);
