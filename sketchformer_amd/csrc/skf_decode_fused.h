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
};

bool skf_decode_fused_supported(int d, int H, int F, int Le, int N, int Vout);
int skf_decode_fused_launch(const SkfDecodeFused& p, hipStream_t st);

// SkfSampling as the public entries take it: struct_size, temperature > 0, top_k >= 0, 0 < top_p <= 1 (SKF_EINVAL otherwise)
int skf_sampling_check(const SkfSampling* s);

// skf_attention_decode plus an optional copy of the softmax rows: attn (B, H, attn_rows, attn_ld), row *step_dev of every
// (sample, head) = the Lk probabilities, then zeros up to attn_ld (attn non-null needs step_dev).
int skf_attention_decode_w(const float* Q, int ldq, const float* K, const float* V, int ld_kv, long long kv_batch_stride,
                           const unsigned char* key_mask, int key_mask_ld, const int* key_limit, int key_limit_all, int B, int H,
                           int Lk, int dh, float* O, int ldo, const int* step_dev, const float* K_new, const float* V_new, int ld_new,
                           int limit_from_step, float* attn, int attn_rows, int attn_ld, hipStream_t stream);
