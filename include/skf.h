/* skf.h - C ABI of libskf.so, the MI355X (gfx950) implementation of the
 * sketch-transformer-tf2 training hot path of leosampaio/sketchformer.
 *
 * The reference has no native layer: every entry point below replaces arithmetic
 * that the reference delegates to TensorFlow 2.1 / Keras from the cited Python call
 * site (paths relative to the reference repository).  A reference-side binding
 * (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers unless the
 *    parameter name ends in _host.  Activations are row-major (B, L, features).
 *  - the caller owns every buffer; kernels never allocate.  Scratch is passed as
 *    (workspace, workspace_bytes); sizes come from the *_workspace_bytes queries.
 *  - launches are asynchronous on `stream` (a hipStream_t cast to void*), re-entrant,
 *    and keep no global state besides a thread-local error string (the opt-in launch
 *    profiler below is a measurement facility of the calling process, off by default).
 *    The library reads no environment variable and has no build-time switch: there is one
 *    build, the shipped one.
 *  - return 0 on success, negative on error (never throws across the ABI);
 *    skf_last_error() describes the last failure on the calling thread.
 */
#ifndef SKF_H_
#define SKF_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* skf_stream_t; /* hipStream_t */

#define SKF_OK 0
#define SKF_EINVAL (-1)       /* bad argument */
#define SKF_EUNSUPPORTED (-2) /* valid in the reference, not implemented here */
#define SKF_EHIP (-3)         /* HIP runtime / launch failure */

const char* skf_last_error(void);
int skf_version(void);
/* name of the device the library will launch on + number of visible devices (host query) */
int skf_device_info(char* name_host, size_t name_len, int* n_devices_host);

/* Per-launch timing with HIP events on the launch stream (bench.py's roofline leg).  enable(1) clears the
 * records and starts recording every kernel launch made through this library on the calling process;
 * report() synchronises the recorded events and writes one JSON array
 * [{"tag","count","ms","flops","bytes"}...] (algorithmic flops / bytes summed over the launches of a tag). */
int skf_profiler_enable(int on);
int skf_profiler_report(char* buf_host, size_t len);

/* ------------------------------------------------------------------ Dense
 * tf.keras.layers.Dense forward / dgrad / wgrad (+bias grad).
 * builders/layers/transformer.py:154-158,196-197; models/sketchformer.py:85-104.
 *   C[M,N] (+)= opA(A)[M,K] . opB(B)[K,N] (+bias) (act) (relu mask)
 *   a_kcontig: 1 = A stored [M][K] (lda = row stride), 0 = A stored [K][M]
 *   b_kcontig: 0 = B stored [K][N] (ldb = row stride), 1 = B stored [N][K]
 *   act: 0 none, 1 relu, 2 tanh;  relu_src (optional, ld_relu): C = 0 where relu_src <= 0
 *   splits > 1 (or bias_grad != NULL): split-K through `workspace`; bias_grad[n] = sum_k B[k][n]
 *   (the bias gradient of a wgrad call, B stored [K][N]); no fused epilogue on that path. */
/* `precision` - the arithmetic of a Dense matmul (an argument of every entry that multiplies, and a field of SkfConfig):
 * SKF_PREC_F32 (0)    = v_mfma_f32_16x16x4_f32 on the fp32 operands (bit-for-bit a k-ordered fmaf chain);
 * SKF_PREC_BF16X6 (6) = every fp32 operand split exactly into three bf16 pieces, the six largest piece products summed
 *     in fp32 on the bf16 matrix cores (dropped terms <= 2^-23 |a||b| per product: the size of one fp32 rounding;
 *     against float64 its error is below the fp32-MFMA kernel's: the piece products are exact and the small ones are
 *     summed before the large ones);
 * SKF_PREC_BF16X3 (3) = two pieces / three products (dropped terms <= 2^-15 |a||b|): opt-in fast mode, never a default.
 * Operands and results are fp32 tensors in every mode.  Non-finite operands: an output element is non-finite in the
 * split modes exactly where it is non-finite in mode 0 (an inf operand gives NaN there instead of +-inf: the remainder
 * of inf is inf - inf); finite outputs are unaffected.  fp32 subnormal operands / pieces below the bf16 normal range are
 * flushed by the bf16 matrix cores: absolute error <= 2^-126 per product (tests/test_gpu_ops.py). */
#define SKF_PREC_F32 0
#define SKF_PREC_BF16X3 3
#define SKF_PREC_BF16X6 6
/* May be OR'ed into the `precision` argument of skf_attention_bwd / skf_attention_bwd_rows: take the two-pass backward
 * (skf_attention_bwd2.hip: a dQ pass over query tiles, a dK/dV pass over key tiles, bf16 matrix cores) wherever it is built
 * (head sizes 16 and 32, Lq, Lk <= 512, split modes) even where the dispatch would pick the one-pass kernel (head size 16). */
#define SKF_ATTN_TWO_PASS 0x100
size_t skf_gemm_workspace_bytes(int M, int N, int K, int splits, int with_bias_grad);
int skf_gemm_default_splits(int M, int N, int K);
int skf_gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                 float* C, int ldc, const float* bias, int act, const float* relu_src, int ld_relu, int accumulate,
                 int splits, float* bias_grad, int bias_grad_accumulate, void* workspace, size_t workspace_bytes,
                 int precision, skf_stream_t stream);

/* wgrad split into its two phases so that a caller can run MANY wgrads and reduce all their slabs with one launch:
 * skf_gemm_wgrad_partial = the partial-tile kernel only (A = X [K][M], B = dY [K][N]; slab layout
 * [splits][M][N] followed by [splits][N] column sums), skf_splitk_reduce_batch = one launch over a DEVICE array of
 * descriptors whose block_begin fields are the running sum of skf_splitk_reduce_blocks(M, N).
 * Contract of one descriptor.  The launch cannot check a device array.  Every descriptor with a bias gradient that the model
 * builds goes through ReduceBatch::add on the host (skf_model_sched.hip), which refuses one that breaks the bias_grad rule below, so
 * the seam group cannot be reached from a train step (tests/test_cabi_cpu.py keeps the refusal in add and the other tables free
 * of bias gradients); a caller of this entry point owes the same check.
 *   - C = sum over the splits (never accumulated), ldc >= N.
 *   - bias_grad != NULL: the [splits][N] column sums follow the tiles; slab must be 16-byte aligned and M*N a multiple of 4 -
 *     the kernel reads float4 groups of [M*N | N] and has no scalar path, a group astride the seam would sum the wrong addresses.
 *   - bias_grad == NULL: slab needs 4-byte alignment only and any M*N is accepted (the 1 x L partials of the expander and the
 *     pooling: rows of odd length, blocks that start at any float - float4 loads at 4-byte granularity, which gfx950 global
 *     loads allow).
 *   - the float4 group that holds the last element is read whole for every split: when M*N (and, with a bias gradient, N) is not a
 *     multiple of 4 the launch READS up to 12 bytes past the last split's tile (column-sum row); the values are discarded, the
 *     bytes must be mapped (the model's slabs lie inside its workspace arena).  Nothing is written outside C / bias_grad.
 * skf_splitk_reduce (one slab) has a scalar path for N % 4 != 0, reads nothing past the slab and refuses M*N % 4 != 0. */
typedef struct SkfReduceDesc {
  const float* slab; float* C; float* bias_grad; /* bias_grad may be NULL */
  int32_t splits, M, N, ldc, block_begin, pad;
} SkfReduceDesc;
int skf_gemm_wgrad_partial(int M, int N, int K, const float* A, int lda, const float* B, int ldb, int splits,
                           int with_bias_grad, float* slab, size_t slab_bytes, int* splits_used_host, int precision,
                           skf_stream_t stream);
/* ---- rows that are known to be zero (decoder-side backward of a padded batch, token mode) ----
 * The masked cross-entropy (builders/losses.py; models/sketchformer.py:313-349) gives padded target positions a zero
 * gradient and the decoder is causal, so every decoder-side gradient row at or behind a sample's last unmasked position
 * is exactly zero.  skf_target_live_len: live_len[b] = 1 + last t < Ld with tar[b][t + 1] != 0 (tar = the (B, tar_ld)
 * int64 target tokens, decoder row t is trained on tar[b][t + 1]).  skf_row_blocks_build: the blocks of `granule`
 * consecutive rows of the flattened (B * rows_per_sample) rows, as {n_live, n_blocks, live ids ascending, dead ids
 * ascending, one 0/1 live flag per block in block order} (skf_row_blocks_bytes bytes).  skf_gemm_f32_rows (dgrad form, A [M][K], granule 16: rows of A in dead blocks
 * are zero -> their C rows are stored as zeros without being computed, or left alone when accumulating) and
 * skf_gemm_wgrad_partial_rows (granule 32: contraction rows in dead blocks are zero in B = dY and are not visited) are
 * EXACT: what is skipped is x * 0.  Kernels other than the split-arithmetic weight-stationary ones ignore the list. */
int skf_target_live_len(const long long* tar, int tar_ld, int B, int Ld, int* live_len, skf_stream_t stream);
size_t skf_row_blocks_bytes(int rows, int granule);
int skf_row_blocks_build(const int* live_len, int B, int rows_per_sample, int granule, int* blocks, skf_stream_t stream);
int skf_gemm_f32_rows(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                      float* C, int ldc, const float* bias, int act, const float* relu_src, int ld_relu, int accumulate,
                      int splits, float* bias_grad, int bias_grad_accumulate, void* workspace, size_t workspace_bytes,
                      int precision, const int* row_blocks, int row_block_rows, skf_stream_t stream);
/* ReLU sign bits (ffn: builders/layers/transformer.py:196-197 Dense(dff, relu) -> Dense(d); its tape gradient multiplies
 * d(hidden) by relu'(hidden)).  A forward launch with act = relu can leave ONE BIT per output element ("> 0") in
 * relu_bits_out, in the layout of its own tiles, and the input-gradient launch of the same (M, N, K) reads relu_bits_in
 * instead of the hidden tensor (relu_src): identical results, 1/32 of the bytes.  Exists where the split-arithmetic
 * weight-stationary kernel takes the launch: skf_gemm_relu_bits_bytes returns the buffer size (64-byte aligned buffer), or 0
 * when the shape has no such path - then pass NULL / use relu_src; bits on an unsupported launch are an error. */
size_t skf_gemm_relu_bits_bytes(int M, int N, int K, int precision);
int skf_gemm_f32_bits(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                      float* C, int ldc, const float* bias, int act, const float* relu_src, int ld_relu, int accumulate,
                      int splits, float* bias_grad, int bias_grad_accumulate, void* workspace, size_t workspace_bytes,
                      int precision, const int* row_blocks, int row_block_rows, void* relu_bits_out, const void* relu_bits_in,
                      skf_stream_t stream);
/* Dense + residual + dropout + LayerNorm in ONE launch: the reference's `layernorm1(x + dropout1(attn_output))`
 * (builders/layers/transformer.py:216-224 EncoderLayer.call, :258-272 DecoderLayer.call) where attn_output is the MultiHeadAttention
 * output projection `self.dense(concat_attention)` (:186):
 *   z = x + dropout(A[M,K] . W[K,N] + bias, rate, site);  out = (z - mean) * rstd * gamma + beta;  stats[row] = (mean, rstd)
 * with the arithmetic, the dropout mask and the epsilon (1e-6) of skf_gemm_f32 followed by skf_layernorm_residual_fwd (z is
 * bit-identical to that pair's; mean / rstd are summed in a different order).  z, out and x are row-major with pitch N.  Exists where
 * one workgroup of the split-arithmetic weight-stationary kernel owns whole output rows: skf_gemm_ln_residual_supported
 * (K = N = 128, precision != SKF_PREC_F32); anything else is an error - use the two calls. */
int skf_gemm_ln_residual_supported(int M, int N, int K, int precision);
int skf_gemm_ln_residual_f32(int M, int N, int K, const float* A, int lda, const float* W, int ldw, const float* bias,
                             const float* x, const float* gamma, const float* beta, float* z, float* out, float* stats,
                             float rate, unsigned site, const void* step_state, int precision, skf_stream_t stream);
/* The feed-forward block of a layer in ONE launch per direction: the reference's `point_wise_feed_forward_network`
 * (builders/layers/transformer.py:194-198: Dense(dff, relu) -> Dense(d_model)) together with the `layernorm(out + dropout(ffn(out)))`
 * that wraps it in EncoderLayer.call (:221-224) / DecoderLayer.call (:270-272), and the tape gradient of the two Dense layers:
 *   forward:   h = relu(x[M,d] . W1[d,dff] + b1);  y = h . W2[dff,d] + b2;  z = x + dropout(y, rate, site);
 *              out = (z - mean) * rstd * gamma + beta;  stats[row] = (mean, rstd);  relu_bits_out = sign bits of h
 *   backward:  dh = (dy[M,d] . W2^T) o relu'(h)  (from the sign bits);  dx (+)= dh . W1^T
 * with the split arithmetic of skf_gemm_f32 (SKF_PREC_BF16X6 / BF16X3), the dropout mask of skf_layernorm_residual_fwd and its
 * LayerNorm arithmetic; h / dh are written in full (the weight gradients read them), never read back.  The weights are read from
 * PRE-SPLIT images in the kernel's MFMA operand order: skf_ffn_weight_images builds n of them in one launch (image k from
 * W1[k] [d][dff] pitch ld1[k], W2[k] [dff][d] pitch ld2[k]; transpose[k] = 0: the forward's image, 1: the backward's;
 * skf_ffn_image_bytes each, 16-byte aligned) - rebuild them whenever the weights change (once per optimizer step).  Exists for
 * d = 128, dff = 512 in the split modes (skf_ffn_fused_supported; anything else is an error - use the separate calls).
 * row_blocks (backward, optional): the 16-row block list of skf_row_blocks_build - dead blocks have dy == 0: their dh rows are
 * stored as zeros, their dx rows left alone (accumulate) or zeroed. */
int skf_ffn_fused_supported(int M, int d, int dff, int precision);
size_t skf_ffn_image_bytes(int d, int dff, int precision);
size_t skf_ffn_relu_bits_bytes(int M, int d, int dff, int precision);
int skf_ffn_weight_images(int n, const float* const* W1, const int* ld1, const float* const* W2, const int* ld2,
                          const int* transpose, void* const* images, int d, int dff, int precision, skf_stream_t stream);
int skf_ffn_fused_fwd_f32(int M, int d, int dff, const float* x, const void* image, const float* b1, const float* b2,
                          float* h, void* relu_bits_out, const float* gamma, const float* beta, float* z, float* out,
                          float* stats, float rate, unsigned site, const void* step_state, int precision, skf_stream_t stream);
int skf_ffn_fused_bwd_f32(int M, int d, int dff, const float* dy, const void* image_t, const void* relu_bits_in,
                          float* dh, float* dx, int accumulate, const int* row_blocks, int row_block_rows,
                          int precision, skf_stream_t stream);
/* The forward launch going one step further: proj_out[M, proj_n] = out . Wp + proj_bias for the Dense that consumes the block's
 * LayerNorm output - the NEXT layer's fused q|k|v projection (builders/layers/transformer.py:154-158, 216-217; proj_n = 384) or a
 * query projection (128) - with proj_image = skf_dense_weight_images(Wp [d][proj_n], transpose = 0).  Same arithmetic as
 * skf_gemm_f32 on `out`; everything else as skf_ffn_fused_fwd_f32. */
int skf_ffn_fused_fwd_proj_f32(int M, int d, int dff, const float* x, const void* image, const float* b1, const float* b2,
                               float* h, void* relu_bits_out, const float* gamma, const float* beta, float* z, float* out,
                               float* stats, float rate, unsigned site, const void* step_state, const void* proj_image,
                               const float* proj_bias, int proj_n, float* proj_out, int precision, skf_stream_t stream);
/* The forward launch in its general form: the feed-forward block with an optional LEADING stage and an optional CHAINED projection.
 * Leading stage (pre_image != NULL): the launch starts at the attention output a (= x [M, d]):
 *   pre_z = pre_residual + dropout(a . Wo + pre_bias, rate, pre_site);  pre_out = LayerNorm(pre_z; pre_gamma, pre_beta);  pre_stats = (mean, rstd)
 * - the MultiHeadAttention output projection with its residual LayerNorm (builders/layers/transformer.py:186, 216-224 / 262-268), i.e.
 * skf_gemm_ln_residual_f32 - and pre_out is the block's input and residual (pre_image = skf_dense_weight_images(Wo [d][d], transpose 0)).
 * Chained projection (proj_image != NULL): as skf_ffn_fused_fwd_proj_f32.  struct_size = sizeof(SkfFfnBlockFwd).
 * image == NULL (with pre_image and proj_image): NO feed-forward block - the leading stage followed by the projection of ITS LayerNorm
 * output, proj_out = pre_out . Wp + proj_bias: the decoder's self-attention tail with the cross-attention query projection behind it
 * (builders/layers/transformer.py:258-262); b1, b2, h, relu_bits_out, gamma, beta, z, out, stats, site are not used. */
typedef struct SkfFfnBlockFwd {
  uint32_t struct_size; int32_t M, d, dff, precision;
  const float* x; const void* image; const float* b1; const float* b2; float* h; void* relu_bits_out;
  const float* gamma; const float* beta; float* z; float* out; float* stats;
  float rate; uint32_t site; const void* step_state;
  const void* pre_image; const float* pre_bias; const float* pre_residual; const float* pre_gamma; const float* pre_beta;
  float* pre_z; float* pre_out; float* pre_stats; uint32_t pre_site; int32_t proj_n;
  const void* proj_image; const float* proj_bias; float* proj_out;
} SkfFfnBlockFwd;
int skf_ffn_block_fwd_f32(const SkfFfnBlockFwd* block, skf_stream_t stream);
/* The backward launch starting one step earlier, at the gradient `dout` of the LayerNorm that closes the block
 * (out = LayerNorm(z), z = x + dropout(ffn(x))): dz = LayerNorm'(dout) from (z, stats, gamma) with the arithmetic of
 * skf_layernorm_residual_bwd, dy = dropout'(dz) (written: the second Dense's weight gradient reads it), dh as above, and
 * dx = dz + dh . W1^T (the residual path added in registers; dx is written, not accumulated).  dgamma / dbeta leave as
 * skf_ffn_fused_ln_partials(M) partial row pairs [n][2][d] in ln_partials - sum them with skf_splitk_reduce(ln_partials, n, 1, 2 * d,
 * ...) or ride them in a skf_splitk_reduce_batch descriptor like the LayerNorm launch's partials.  Dead row blocks (row_blocks):
 * dout == 0 there; their dy, dh and dx rows are stored as zeros. */
int skf_ffn_fused_ln_partials(int M);
int skf_ffn_fused_bwd_ln_f32(int M, int d, int dff, const float* dout, const float* z, const float* stats, const float* gamma,
                             float rate, unsigned site, const void* step_state, const void* image_t, const void* relu_bits_in,
                             float* dy, float* dh, float* dx, float* ln_partials, size_t ln_partials_bytes,
                             const int* row_blocks, int row_block_rows, int precision, skf_stream_t stream);
/* Pre-split operand images in general: image j of B_j [K][N] (K % 32 == 0, N % 16 == 0; transpose[j] = 0: B[k][n] = src[k * ld + n],
 * 1: B[k][n] = src[n * ld + k]), skf_dense_image_bytes(K, N, precision) bytes each, all in one launch per 40 images. */
size_t skf_dense_image_bytes(int K, int N, int precision);
int skf_dense_weight_images(int n, const float* const* src, const int* ld, const int* transpose, const int* K, const int* N,
                            void* const* images, int precision, skf_stream_t stream);
/* The backward of `out = LayerNorm(x + dropout(Dense(a)))` - the MultiHeadAttention output projection with the residual LayerNorm
 * behind it (builders/layers/transformer.py:186, 216-224, 258-268) - from the gradient of `out` to the gradient of `a` in ONE launch:
 *   dz = LayerNorm'(dout) (written: the residual path's gradient), dy = dropout'(dz) (written: the Dense's weight gradient reads it),
 *   da = dy[M,d] . W^T   (image_t = the transposed image of W [d][d]: skf_dense_weight_images(.., transpose = 1, K = d, N = d))
 * with the arithmetic of skf_layernorm_residual_bwd followed by skf_gemm_f32; dgamma / dbeta as skf_layernorm_bwd_dgrad_partials(M)
 * partial row pairs [n][2][d] (see skf_ffn_fused_bwd_ln_f32).  Exists for d = 128 in the split modes.  row_blocks: 16-row blocks,
 * dead blocks have dout == 0 and get zero rows in dz, dy and da. */
int skf_layernorm_bwd_dgrad_supported(int M, int d, int precision);
int skf_layernorm_bwd_dgrad_partials(int M);
int skf_layernorm_bwd_dgrad_f32(int M, int d, const float* dout, const float* z, const float* stats, const float* gamma,
                                float rate, unsigned site, const void* step_state, const void* image_t, float* dz, float* dy,
                                float* da, float* ln_partials, size_t ln_partials_bytes, const int* row_blocks,
                                int row_block_rows, int precision, skf_stream_t stream);
/* the same with a LEADING product: the gradient of `out` is dout + lead_a[M,d] . Wl^T (lead_image_t = the transposed image of Wl [d][d]) -
 * the input gradient of a Dense that reads `out` (the decoder's cross-attention query projection, builders/layers/transformer.py:258-262),
 * formed in the launch instead of being accumulated into dout by a GEMM launch of its own; lead_a == NULL: skf_layernorm_bwd_dgrad_f32 */
int skf_layernorm_bwd_dgrad_lead_f32(int M, int d, const float* dout, const float* lead_a, const void* lead_image_t, const float* z,
                                     const float* stats, const float* gamma, float rate, unsigned site, const void* step_state,
                                     const void* image_t, float* dz, float* dy, float* da, float* ln_partials, size_t ln_partials_bytes,
                                     const int* row_blocks, int row_block_rows, int precision, skf_stream_t stream);
int skf_gemm_wgrad_partial_rows(int M, int N, int K, const float* A, int lda, const float* B, int ldb, int splits,
                                int with_bias_grad, float* slab, size_t slab_bytes, int* splits_used_host, int precision,
                                const int* row_blocks, int row_block_rows, skf_stream_t stream);
/* the partial-tile kernels of up to 8 weight gradients in one launch (a transformer layer's, issued together); a HOST array,
 * splits_used is written per problem; problems the split-arithmetic kernel cannot take fall back to one launch each */
typedef struct SkfWgradProblem {
  const float* A; const float* B; float* slab; size_t slab_bytes; const int* row_blocks;   /* row_blocks may be NULL */
  int32_t M, N, K, lda, ldb, splits, with_bias_grad, row_block_rows, splits_used, pad;
} SkfWgradProblem;
int skf_gemm_wgrad_partial_group(SkfWgradProblem* probs, int n, int precision, skf_stream_t stream);
/* one slab ([splits][M][N] then [splits][N] when bias_grad != NULL) -> C (+)= sum, bias_grad (+)= column sums */
int skf_splitk_reduce(const float* slab, int splits, int M, int N, float* C, int ldc, int accumulate, float* bias_grad,
                      int bias_grad_accumulate, skf_stream_t stream);
int skf_splitk_reduce_blocks(int M, int N);
int skf_splitk_reduce_batch(const SkfReduceDesc* descs_dev, int ndesc, int total_blocks, skf_stream_t stream);

/* ------------------------------------------------------------------ attention
 * builders/utils.py:71-105 scaled_dot_product_attention + the head split / merge of
 * builders/layers/transformer.py:160-186 + the masks of builders/utils.py:35-68.
 * Q (B,Lq,ldq) K,V (B,Lk,ld*) O (B,Lq,ldo); head h = columns [h*dh,(h+1)*dh).
 * key_mask: (B, key_mask_ld) bytes, 1 = padded key (create_padding_mask), may be NULL.
 * precision != SKF_PREC_F32: the score products of the dh = 16 kernels run on the bf16 matrix cores with split operands.
 * causal: add the look-ahead mask (needs Lq == Lk).  stats: (B,H,Lq,2) row max of the base-2 logits
 * (q.k * log2(e)/sqrt(dh)) and 1/row-sum - opaque to the caller, kept for the backward.  dh in {16,32,64}: Lk <= 512 and one
 * head's operands in 160 KB of LDS, i.e. forward Lk <= 288 at dh 64; backward Lq <= 224 at dh 64 and Lq <= 448 at dh 32 (512 at
 * dh 16).  Any other dh <= 128: plain fp32 kernels, Lq, Lk <= 1024.  Anything else is refused before a launch. */
int skf_attention_fwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                      const unsigned char* key_mask, int key_mask_ld, int causal, int B, int H, int Lq, int Lk, int dh,
                      float* O, int ldo, float* stats, int precision, skf_stream_t stream);
int skf_attention_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                      const float* dO, int lddo, const float* stats, const unsigned char* key_mask, int key_mask_ld,
                      int causal, int B, int H, int Lq, int Lk, int dh, float* dQ, int lddq, float* dK, int lddk,
                      float* dV, int lddv, int precision, skf_stream_t stream);
/* the same with per-sample live query counts (skf_target_live_len): query rows >= q_live_len[b] have dO == 0 exactly; the
 * one-pass kernel neither stages nor visits their tiles and stores zeros into their dQ rows (the two-pass kernel finds
 * all-zero dO tiles by itself) */
int skf_attention_bwd_rows(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                           const float* dO, int lddo, const float* stats, const unsigned char* key_mask, int key_mask_ld,
                           int causal, int B, int H, int Lq, int Lk, int dh, float* dQ, int lddq, float* dK, int lddk,
                           float* dV, int lddv, int precision, const int* q_live_len, skf_stream_t stream);
/* Padded batches: a (sample, head) workgroup costs what its sample's length makes it cost, and consecutive workgroups of an XCD are
 * handed to its four shader engines in turn and never leave them - so the engine that draws the long samples finishes last.
 * skf_sample_order: order[0..B) = the samples sorted by the number of UNMASKED positions in up to two padding-mask matrices (either may
 * be NULL), most first, stable (B <= 4096).  The *_ordered forms take that list (or NULL = the plain numbering) and deal the sorted samples over the
 * 8 XCDs, heaviest first, the heads of a sample over the engines of its XCD; used when B is a multiple of 8, ignored otherwise and by the
 * plain fp32 kernels of other head sizes.  The numbering never changes a result bit.  sample_order must be a PERMUTATION of [0, B) in device
 * memory (what skf_sample_order writes); the kernels do not verify it - entries are clamped into [0, B), so a malformed list cannot touch
 * memory outside the tensors, but it computes some samples twice and leaves the outputs of others unwritten.  Measured (B 128, H 8, L 200, 58 % padding): the three
 * backward calls of a layer 168 -> 143 us, the forward calls 98 -> 90 us (profiles/r05o_attn_order.txt). */
int skf_sample_order(const unsigned char* mask_a, int lda, int La, const unsigned char* mask_b, int ldb, int Lb, int B, int* order,
                     skf_stream_t stream);
int skf_attention_fwd_ordered(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                              const unsigned char* key_mask, int key_mask_ld, int causal, int B, int H, int Lq, int Lk, int dh,
                              float* O, int ldo, float* stats, int precision, const int* sample_order, skf_stream_t stream);
int skf_attention_bwd_ordered(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                              const float* dO, int lddo, const float* stats, const unsigned char* key_mask, int key_mask_ld,
                              int causal, int B, int H, int Lq, int Lk, int dh, float* dQ, int lddq, float* dK, int lddk,
                              float* dV, int lddv, int precision, const int* q_live_len, const int* sample_order, skf_stream_t stream);
/* The second return value of scaled_dot_product_attention (builders/utils.py:105: `return output, attention_weights`):
 * W (B,H,Lq,Lk) = softmax(q.k/sqrt(dh) + mask * -1e9) over the keys, same mask arguments as skf_attention_fwd.  Only the builders
 * front-end calls it, on request (the train step of the reference drops the weights: models/sketchformer.py:140-145); plain fp32
 * kernel, any dh <= 128, Lq, Lk <= 1024. */
int skf_attention_weights(const float* Q, int ldq, const float* K, int ldk, const unsigned char* key_mask, int key_mask_ld,
                          int causal, int B, int H, int Lq, int Lk, int dh, float* W, skf_stream_t stream);
/* builders/utils.py:71-105 scaled_dot_product_attention with ANY float mask broadcastable to (B,H,Lq,Lk) (`:96-97`:
 * `scaled_attention_logits += (mask * -1e9)` - the mask is ADDED, a fractional value lowers a logit, it does not remove the key).
 * mask may be NULL; mask_stride_b / _h / _q are ELEMENT strides of the sample / head / query axes (0 = broadcast), the key axis has
 * unit stride.  O (B,Lq,H*dh) with row stride ldo; W = the (B,H,Lq,Lk) weights or NULL.  Plain fp32 kernel of skf_generic.hip (one
 * wave per query row: correct, not fast) - the padding and padding + look-ahead masks the model builds go to skf_attention_fwd as
 * bytes; the front-end (builders.utils.scaled_dot_product_attention) routes every other mask here instead of refusing it. */
int skf_attention_fwd_float_mask(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* mask,
                                 long mask_stride_b, long mask_stride_h, long mask_stride_q, int B, int H, int Lq, int Lk, int dh,
                                 float* O, int ldo, float* W, skf_stream_t stream);
/* Row means behind LossManager.add_mean_loss / add_mae_loss / add_mse_loss (builders/losses.py:68-75; tf.keras.losses.MAE / MSE
 * reduce the LAST axis): out[r] = mean_c a[r][c] (mode 0), mean_c |a - b| (mode 1), mean_c (a - b)^2 (mode 2); a, b (rows, cols)
 * contiguous. */
int skf_row_mean(const float* a, const float* b, long rows, int cols, int mode, float* out, skf_stream_t stream);

/* ------------------------------------------------------------------ embedding stage
 * Encoder.call / Decoder.call head, builders/layers/transformer.py:288-296, 325-334:
 * out = Dropout(Embedding(tok) * sqrt(d) + pos[:L]).  tokens (B, tok_ld) int64 (first L used). */
int skf_embed_fwd(const long long* tokens, int tok_ld, int B, int L, const float* table, int vocab, int d,
                  const float* pos, float* out, float rate, unsigned site, const void* step_state, skf_stream_t stream);
/* dtable (vocab,d) must be zeroed by the caller; receives the dense embedding gradient. */
int skf_embed_bwd(const long long* tokens, int tok_ld, int B, int L, const float* dx, int vocab, int d, float* dtable,
                  float rate, unsigned site, const void* step_state, skf_stream_t stream);
/* The same gradient without pre-zeroed table and (almost) without atomics, in two launches: skf_embed_sort depends on the
 * tokens only (counting sort of the B*L positions by id into `ws`, one workgroup; rows of ids that need more than one
 * 256-position chunk are zeroed in `zero_table` when it is not NULL), skf_embed_bwd_sorted then writes EVERY row of
 * dtable (zeros for unused ids). */
size_t skf_embed_sort_workspace_bytes(int B, int L, int vocab);
int skf_embed_sort(const long long* tokens, int tok_ld, int B, int L, int vocab, float* zero_table, int d, void* ws,
                   size_t ws_bytes, skf_stream_t stream);
int skf_embed_bwd_sorted(const void* ws, int B, int L, const float* dx, int vocab, int d, float* dtable, float rate,
                         unsigned site, const void* step_state, skf_stream_t stream);
/* key padding mask bytes (create_padding_mask, builders/utils.py:35-43): out[b][t] = tokens[b][t]==0 */
int skf_padding_mask(const long long* tokens, int tok_ld, int B, int L, unsigned char* out, skf_stream_t stream);

/* ------------------------------------------------------------------ residual + LayerNorm
 * out = LayerNormalization(eps=1e-6)(x + Dropout(y)); builders/layers/transformer.py:217-222,247-260.
 * y is overwritten with z = x + Dropout(y); stats (rows,2) = mean, rstd. */
int skf_layernorm_residual_fwd(const float* x, float* y_inout_z, const float* gamma, const float* beta, float* out,
                               float* stats, int rows, int d, float rate, unsigned site, const void* step_state,
                               skf_stream_t stream);
size_t skf_layernorm_bwd_workspace_bytes(int rows, int d);
/* dz = d(x + drop(y)); dy = dz * dropout mask (only written when rate > 0; with rate == 0 dy == dz). */
/* dgamma == dbeta == NULL: only the per-workgroup partials are written, workspace = [g][2][d] floats with
 * g = skf_layernorm_bwd_workspace_bytes(rows, d) / (8*d) (row 2k = dgamma part, as one [g][2d] matrix); the caller
 * column-sums them later (the train step batches all of them into its split-K reduction launch). */
int skf_layernorm_residual_bwd(const float* dout, const float* z, const float* stats, const float* gamma, float* dz,
                               float* dy, float* dgamma, float* dbeta, int rows, int d, float rate, unsigned site,
                               const void* step_state, void* workspace, size_t workspace_bytes, skf_stream_t stream);
/* rows = B * rows_per_sample; row t of sample b with t >= live_len[b] has dout == 0 exactly (skf_target_live_len): it is not
 * read, zeros are stored (d <= 256; wider rows take the dense kernel) */
int skf_layernorm_residual_bwd_rows(const float* dout, const float* z, const float* stats, const float* gamma, float* dz,
                                    float* dy, float* dgamma, float* dbeta, int rows, int d, float rate, unsigned site,
                                    const void* step_state, void* workspace, size_t workspace_bytes, const int* live_len,
                                    int rows_per_sample, skf_stream_t stream);
int skf_colsum(const float* in, int nrows, int ld, int ncols, float* out, int accumulate, skf_stream_t stream);

/* ------------------------------------------------------------------ loss heads + metrics
 * Sparse softmax CE from logits, fused accuracy + in-place gradient.
 * builders/losses.py:26-41 (mask_pad=1: loss*(target!=0), mean over ALL rows -> scale = weight/rows),
 * builders/losses.py:21-24 (mask_pad=0), builders/keras_metrics.py:25 (first-index argmax == target).
 * target element for row r: target[(r / tgt_cols) * tgt_ld + (r % tgt_cols) + tgt_off].
 * probs_out (rows,ncls) optional (classify_layer's softmax output, models/sketchformer.py:99). */
int skf_softmax_ce(float* logits, int ld, int rows, int ncls, const long long* target, int tgt_ld, int tgt_cols,
                   int tgt_off, int mask_pad, float scale, float* row_loss, float* row_hit, float* probs_out,
                   int write_grad, skf_stream_t stream);
/* metrics (32 floats): [0..4] this step recon_loss, recon_acc, class_loss, class_acc, total_loss;
 * [8..12] running totals, [16..20] running counts (Keras Mean / SparseCategoricalAccuracy). */
int skf_metrics_update(const float* recon_loss, const float* recon_hit, int recon_rows, float recon_weight,
                       const float* class_loss, const float* class_hit, int class_rows, float class_weight,
                       const float* recon_scalar /* continuous mode: the already reduced recon loss, else NULL */,
                       float* metrics, skf_stream_t stream);

/* ------------------------------------------------------------------ continuous stroke-5 mode (use_continuous_data=True)
 * x (B, x_ld_rows, 5) float32 stroke-5 rows; the first L rows of every sample are used.
 * builders/utils.py:35-43 (pad bit), builders/layers/transformer.py:276,288-296 (embedding = Dense(5->d)),
 * builders/losses.py:43-66 (location MSE + GLOBAL mean pen-state CE, masked, mean over all positions). */
int skf_padding_mask_continuous(const float* x, int x_ld_rows, int B, int L, unsigned char* out, skf_stream_t stream);
int skf_embed_continuous_fwd(const float* x, int x_ld_rows, int B, int L, const float* W, const float* bias, int d,
                             const float* pos, float* out, float rate, unsigned site, const void* step_state,
                             skf_stream_t stream);
size_t skf_embed_continuous_bwd_workspace_bytes(int rows, int d);
/* d <= 682: the backward keeps [4 waves][6][d] floats in LDS (4 * 6 * d * 4 bytes <= 64 KB); a wider d is refused */
int skf_embed_continuous_bwd(const float* x, int x_ld_rows, int B, int L, const float* dx, int d, float* dW, float* dbias,
                             float rate, unsigned site, const void* step_state, void* workspace, size_t workspace_bytes,
                             skf_stream_t stream);
/* pred (rows,5) is overwritten with the gradient when write_grad; target row r =
 * target[(r / tgt_cols) * tgt_ld_rows + r % tgt_cols + tgt_off]; scalars (4 floats): sum(loc*mask), sum(ce),
 * sum(mask), weighted loss. */
int skf_continuous_loss(float* pred_inout_grad, const float* target, int tgt_ld_rows, int tgt_cols, int tgt_off, int rows,
                        float weight, float* row_loc, float* row_ce, float* row_mask, float* scalars, int write_grad,
                        skf_stream_t stream);

/* ------------------------------------------------------------------ bottleneck + expander
 * SelfAttnV1.call after u = tanh(xW+b): builders/layers/transformer.py:70-73. */
int skf_pool_fwd(const float* u, const float* Vw, const float* x, int B, int L, int U, int d, float* a_out, float* emb,
                 skf_stream_t stream);
/* u is overwritten with d(pre-tanh); dx receives a[t]*demb[c]; workspace >= B*U floats */
int skf_pool_bwd(float* u_inout_dpre, const float* Vw, const float* x, const float* a, const float* demb, int B, int L,
                 int U, int d, float* dx, float* dV, void* workspace, size_t workspace_bytes, skf_stream_t stream);
/* DenseExpander.call: builders/layers/transformer.py:370-376. workspace >= 2*B*L floats */
int skf_expander_fwd(const float* emb, const float* w, const float* bias, int B, int L, int d, float* pre,
                     skf_stream_t stream);
int skf_expander_bwd(const float* dpre, const float* emb, const float* w, int B, int L, int d, float* demb,
                     int demb_accumulate, float* dw, float* dbias, void* workspace, size_t workspace_bytes,
                     skf_stream_t stream);

/* ------------------------------------------------------------------ optimizer
 * builders/schedulers.py:13-46 + tf.keras.optimizers.Adam (models/sketchformer.py:112-124,348).
 * step_state is skf_step_state_bytes() of device memory {int64 iterations; float lr, alpha; u32 drop_key, micro}.
 * schedule 0: WarmupDecay p0=d_model, p1=warmup^-1.5; 1: StepDecay p0=init_lr p1=rate p2=steps p3=min_ratio; 2: const p0
 * micro (zero unless gradient accumulation moves it, skf_grad_accumulate) counts the micro-batches already summed into the open
 * optimizer step.  The prologue derives lr and alpha from `iterations` alone and the dropout key from (seed, iterations, micro):
 * micro == 0 gives hash(seed, iterations), the key of a step without accumulation; micro = j > 0 hashes j into that key with a
 * further round, so the micro-steps of one optimizer step draw different masks and none of them draws those of a later step. */
size_t skf_step_state_bytes(void);
int skf_step_prologue(void* step_state, int schedule, float p0, float p1, float p2, float p3, float beta1, float beta2,
                      unsigned seed, skf_stream_t stream);
int skf_step_epilogue(void* step_state, skf_stream_t stream);
/* host helper: the dropout key the prologue writes for (seed, iterations, micro) */
unsigned skf_step_drop_key(unsigned seed, long long iterations, unsigned micro);
int skf_adam_step(float* w, const float* g, float* m, float* v, size_t n, const void* step_state, float grad_scale,
                  float beta1, float beta2, float eps, skf_stream_t stream);
/* tf.keras.optimizers.SGD(lr_schedule, momentum), nesterov=False: velocity = momentum*velocity - lr*g*grad_scale; w += velocity */
int skf_sgd_momentum_step(float* w, const float* g, float* velocity, size_t n, const void* step_state, float grad_scale,
                          float momentum, skf_stream_t stream);
/* Gradient accumulation (skf_accum.hip): dst[i] = a[i] + b[i] over n floats, dst[i] = a[i] with b == NULL.  One fp32 add per
 * element, rounded once - the bits of a host a + b; inf and NaN pass through.  dst may be a or b.  One launch: 16-byte loads and
 * stores, at most 2048 workgroups striding over the buffer, a scalar tail for n % 4; no atomics, no workspace.
 * micro_op: what one thread of the same launch does to step_state's `micro` word - SKF_MICRO_KEEP nothing (step_state may be NULL),
 * SKF_MICRO_NEXT micro += 1, SKF_MICRO_ZERO micro = 0.  n == 0 with a micro_op moves the counter alone (dst, a may be NULL).
 * SKF_EINVAL with a message: dst, a or b not 16-byte aligned, a null dst or a with n > 0, an unknown micro_op, a micro_op other
 * than KEEP without a step state. */
#define SKF_MICRO_KEEP 0
#define SKF_MICRO_NEXT 1
#define SKF_MICRO_ZERO 2
int skf_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* step_state, int micro_op, skf_stream_t stream);
/* Weight averaging (skf_ema.hip): tf.train.ExponentialMovingAverage / tfa.optimizers.MovingAverage without zero-debias.
 * skf_ema_update: shadow[i] -= (shadow[i] - w[i]) * (1 - d) over n floats - three fp32 operations per element, each rounded once,
 * nothing fused: the bits of TensorFlow's assign_moving_average and of a float32 host restatement.  d = decay with num_updates == 0,
 * otherwise min(decay, (1 + n) / (10 + n)) with n = (float)iterations read from step_state BY THE KERNEL (no host read, no launch
 * in front); skf_ema_decay_at is the same fp32 expression on the host.  skip (NULL = never): a device word - the skip flag of the
 * clipped sweeps - with skip[0] != 0 the launch writes nothing.  It writes `shadow` alone, never w, the step state or skip.  One
 * launch: 16-byte loads and stores, at most 2048 workgroups striding over the buffer, a scalar tail for n % 4; no atomics, no
 * workspace; 12 B of traffic per element.
 * skf_buffer_swap: exchanges a and b (n floats each) in place as 16-byte words of bits - NaN payloads survive.  Same launch shape.
 * SKF_EINVAL with a message: a decay that is not finite or not inside (0, 1), pointers not 16-byte aligned, operands that are the
 * same buffer or overlap, num_updates without a step state. */
int skf_weight_average_validate(float decay);
float skf_ema_decay_at(float decay, int num_updates, long long iterations);
int skf_ema_update(float* shadow, const float* w, size_t n, float decay, int num_updates, const void* step_state, const void* skip,
                   skf_stream_t stream);
int skf_buffer_swap(float* a, float* b, size_t n, skf_stream_t stream);

/* y = inverted dropout of x (n floats, y may alias x) with the mask of (step key, site, element index);
 * applied to an upstream gradient it is the backward.  rate 0 = copy. */
int skf_dropout(const float* x, float* y, size_t n, float rate, unsigned site, const void* step_state, skf_stream_t stream);
/* host helper for parity tests: the keep-mask the kernels derive for (drop_key, site) */
int skf_dropout_keep_mask(unsigned drop_key, unsigned site, float rate, size_t n, unsigned char* out_host);

/* ---- single-query attention + token selection of the KV-cached greedy decode ----
 * skf_attention_decode: scaled_dot_product_attention (builders/utils.py:71-105) for ONE query row per (sample, head):
 *   Q (B, H*dh) row stride ldq; K/V rows of sample b start at K + b*kv_batch_stride, row stride ld_kv, Lk rows used;
 *   key_mask (B, key_mask_ld) bytes, 1 = masked (additive -1e9); keys >= key_limit[b] (or key_limit_all if > 0) masked.
 *   Graph-replayable form: step_dev (device int) non-NULL and K_new/V_new (B, ld_new) given -> the number of keys is
 *   *step_dev + 1 (Lk = cache capacity), the newest key/value row is read from K_new/V_new and appended to the cache at
 *   row *step_dev; limit_from_step: keys >= *step_dev + 1 are masked where key_limit is NULL or negative.
 * skf_decode_init: column 0 of the output = SOS (tokens) or (0,0,1,0,0) (continuous); clears the flags (and *step_dev).
 * skf_decode_embed: decoder input of position *step_dev: table[token] (or Dense(5->d) of the stroke-5 row) * sqrt(d) + pos.
 *   A token id outside [0, vocab) takes the row of id 0 here and in the one-launch decode (both decode paths clamp); the training
 *   side's skf_embed_fwd stores a ZERO embedding vector for such an id instead (its backward skips it).
 * skf_decode_select_tokens / _continuous: models/sketchformer.py:285-301 - append argmax (first index on ties) or
 *   (x, y, softmax(pen)); maintain the target padding mask, the sticky EOS flags and done_step (-1 until the stop test
 *   holds).  With step_dev/dyn non-NULL the step, n_valid (dyn[0]) and eos (dyn[1]) are read from device memory and
 *   *step_dev is incremented, so that one captured launch sequence serves every step. */
int skf_attention_decode(const float* Q, int ldq, const float* K, const float* V, int ld_kv, long long kv_batch_stride,
                         const unsigned char* key_mask, int key_mask_ld, const int* key_limit, int key_limit_all, int B,
                         int H, int Lk, int dh, float* O, int ldo, const int* step_dev, const float* K_new,
                         const float* V_new, int ld_new, int limit_from_step, skf_stream_t stream);
int skf_decode_init(long long* tokens, int tok_ld, float* cont, int cont_ld_rows, unsigned char* selfmask, int mask_ld,
                    int* eos_seen, int* done_step, int B, long long sos, int* step_dev, skf_stream_t stream);
int skf_decode_embed(const long long* tokens, const float* cont, int ld, int B, const float* table, int vocab,
                     const float* W, const float* bias, int d, const float* pos, const int* step_dev, float* out,
                     skf_stream_t stream);
int skf_decode_select_tokens(const float* logits, int ld, int B, int V, int n_valid, int step, long long eos,
                             long long* tokens, int tok_ld, unsigned char* selfmask, int mask_ld, int* eos_seen,
                             int* done_step, int* step_dev, const long long* dyn, skf_stream_t stream);
int skf_decode_select_continuous(const float* pred, int ld, int B, int n_valid, int step, float* out, int out_ld_rows,
                                 unsigned char* selfmask, int mask_ld, int* done_step, int* step_dev,
                                 const long long* dyn, skf_stream_t stream);

/* ---- sampled token selection: temperature, top-k and nucleus (top-p) decoding ----
 * The selection rule, for one row of V fp32 logits, temperature > 0, top_k >= 0 (0 = off), 0 < top_p <= 1 (1 = off) and a
 * uniform u in [0, 1):
 *   1. z_j = logit_j / temperature in fp32; m = max z; e_j = exp(z_j - m).
 *   2. top-k: keep j iff z_j >= the k-th largest z (ties at the threshold are all kept; top_k >= V keeps everything);
 *      dropped entries get e_j = 0.
 *   3. nucleus, over what top-k kept, S = the kept mass: keep j iff the mass of kept entries with z_i > z_j is < top_p * S
 *      (ties share one fate, the maximum is always kept).
 *   4. inverse CDF in INDEX order over the survivors, S' their mass: r = u * S'; the token is the smallest surviving j whose
 *      inclusive prefix sum of e exceeds r.
 *   Both cuts are thresholds on z, so the result does not depend on how equal values are ordered.  The kernels hold a mass as
 *   the integer floor(e_j * 2^32): every sum and prefix sum is exact and order-free (no floating-point atomics), r is
 *   floor(u * S') < S', so a token is always found, and the token is a pure function of (row, parameters, u).
 * The random stream: skf_sample_uniform(seed, stream_id, step) = n * 2^-24, n the top 24 bits of three rounds of the 32-bit
 *   hash the dropout masks use; stateless, the same on host and device.  stream_id is a per-row integer of the caller's
 *   choosing: a row's draws depend neither on the batch slot it occupies nor on what else is in the batch.
 * SkfSampling: struct_size = sizeof(SkfSampling) (checked like SkfConfig's); SKF_EINVAL for temperature <= 0, top_k < 0 or
 *   top_p outside (0, 1].
 * skf_decode_sample_tokens: skf_decode_select_tokens with the token of row b drawn by the rule above with
 *   u = skf_sample_uniform(sampling->seed, stream_ids[b], step) instead of maximised; stream_ids: B device ints.  One workgroup
 *   per row holds the row in LDS (V <= 40064, else SKF_EUNSUPPORTED), a second launch does the done_step / step_dev part.
 *   Same padding mask, sticky EOS flags and step_dev / dyn device-side form as skf_decode_select_tokens. */
typedef struct SkfSampling {
  uint32_t struct_size; /* sizeof(SkfSampling) */
  float temperature;    /* > 0; 1 = the model's distribution */
  int32_t top_k;        /* 0 = off */
  float top_p;          /* in (0, 1]; 1 = off */
  uint32_t seed;
} SkfSampling;
float skf_sample_uniform(unsigned seed, unsigned stream_id, unsigned step);
int skf_decode_sample_tokens(const float* logits, int ld, int B, int V, int n_valid, int step, long long eos,
                             long long* tokens, int tok_ld, unsigned char* selfmask, int mask_ld, int* eos_seen,
                             int* done_step, int* step_dev, const long long* dyn, const SkfSampling* sampling,
                             const int* stream_ids, skf_stream_t stream);

/* ---- beam search: the W most likely reconstructions of a sketch ----
 * A batch of B rows decodes n = B / W sketches: rows g W .. g W + W - 1 are the beams of sketch g (1 <= W <= SKF_BEAM_MAX).
 * One position is two launches.  The position kernel gives every row its W best (log p, token) pairs of the row's log-softmax
 * (fp32: one max, one sum of expf in a fixed order), log p descending, then token ascending.  The selection rule of
 * skf_beam_advance then merges the offers of a sketch:
 *   a live beam r offers (score[r] + logp[r][k], token[r][k]) for k < W; a finished beam (it has emitted EOS) offers exactly one
 *   candidate, itself: (score[r], PAD = 0); a beam of score -inf offers nothing finite; NaN ranks as -inf.
 *   The W best offers survive, ordered by score descending, then parent beam ascending, then token ascending.  Survivor r' writes
 *   token [r'][step + 1], mask byte (token == 0), its score, the sticky finished flag, its length (the position of its EOS; for a
 *   live beam the positions emitted so far) and row r' of the next ancestry table.
 * Ancestry: no K/V row, mask byte or token is ever copied.  (row, position) is written once, at step == position; hypothesis r is
 *   the list anc[r][0..step] of the rows ("slots") that hold its positions: anc'[r'][0..step] = anc[parent][0..step],
 *   anc'[r'][step + 1] = r'.  Two tables (2, rows, ancestry_ld): the position `step` reads table step & 1 and writes the other.
 * Scores are fp32 sums in step order and nothing uses a floating-point atomic: two calls are bit-equal.
 * skf_beam_advance: one such merge on caller buffers (device): cand_logp / cand_tok (n W, W); scores, finished, lengths (n W),
 *   updated in place; parent: optional (n W) ints, the parent beam of every survivor.
 * skf_beam_finish: the final order on caller buffers (device).  The W hypotheses of every sketch are ordered by
 *   scores / ((5 + lengths) / 6)^length_alpha descending, then beam index ascending; out_scores (n, W) and out_lengths (n, W) are the
 *   inputs in that order (the raw sums); out_tokens (n, W, T): hypothesis r read through its ancestry row,
 *   tokens[ancestry[r][j]][j] for j < ncols, zeros from ncols on.  ancestry (n W, ancestry_ld): ONE table. */
#define SKF_BEAM_MAX 8
typedef struct SkfBeam {
  uint32_t struct_size; /* sizeof(SkfBeam) */
  int32_t beam_width;   /* W in [1, min(SKF_BEAM_MAX, vocab_size, batch)] */
  float length_alpha;   /* >= 0; final order by score / ((5 + len) / 6)^length_alpha; 0 = the raw sum */
} SkfBeam;
int skf_beam_finish(const float* scores, const int* lengths, const int* ancestry, int ancestry_ld, const long long* tokens,
                    int tok_ld, int n, int beam_width, int ncols, int T, float length_alpha, long long* out_tokens,
                    float* out_scores, int* out_lengths, skf_stream_t stream);
int skf_beam_advance(const float* cand_logp, const int* cand_tok, int n, int beam_width, int step, long long eos,
                     float* scores, int* finished, int* lengths, int* ancestry, int ancestry_ld, long long* tokens,
                     int tok_ld, unsigned char* selfmask, int mask_ld, int* parent, skf_stream_t stream);

/* ------------------------------------------------------------------ bf16 path (BASELINE cfg 5)
 * bf16 storage + v_mfma_f32_32x32x16_bf16 with fp32 accumulation, fp32 master weights / optimizer state (SkfConfig.act_dtype
 * = SKF_ACT_BF16).  `void*` tensors below are bf16 (2 bytes per element, pitches in elements); parameters, statistics,
 * losses and parameter gradients stay fp32.  Same reference lines as the fp32 entries they mirror.
 *
 * Dense (builders/layers/transformer.py:154-158,196-197): C[M][N] (+)= A[M][K] . B_nk[N][K]^T (+bias) (act: 0 none, 1 relu,
 * 2 tanh) (relu mask); both operands contraction-contiguous: the forward passes the [out][in] image of the weight, the input
 * gradient the [in][out] image (skf_cast_weight_bf16 makes both from the fp32 master).  lda / ldb multiples of 8 and
 * >= K rounded up to 8 (pad columns must hold zeros: they take part in the contraction); ldc, N multiples of 4.
 * C_f32: optional fp32 copy of the result. */
int skf_gemm_bf16(int M, int N, int K, const void* A, int lda, const void* B_nk, int ldb, void* C, int ldc, const float* bias,
                  int act, const void* relu_src, int ld_relu, int accumulate, float* C_f32, int ldc_f32, skf_stream_t stream);
/* weight gradient dW[P][Q] = sum_r X[r][P] dY[r][Q] (+ column sums of dY = bias gradient): fp32 partial tiles
 * [splits][P][Q] (+ [splits][Q]) into `slab`, reduced by skf_splitk_reduce_batch like the fp32 path's. */
int skf_gemm_bf16_wgrad_splits(int P, int Q, int R);
size_t skf_gemm_bf16_wgrad_workspace_bytes(int P, int Q, int R, int splits);
int skf_gemm_bf16_wgrad_partial(int P, int Q, int R, const void* X, int ldx, const void* dY, int lddy, int splits,
                                int with_bias_grad, float* slab, size_t slab_bytes, int* splits_used_host, skf_stream_t stream);
/* the same + its reduction into the fp32 gradient dW[P][Q] (row stride ldw) and bias_grad[Q] (may be NULL); workspace >=
 * skf_gemm_bf16_wgrad_workspace_bytes(P, Q, R, skf_gemm_bf16_wgrad_splits(P, Q, R)) (fewer splits are used if it is smaller) */
int skf_gemm_bf16_wgrad(int P, int Q, int R, const void* X, int ldx, const void* dY, int lddy, float* dW, int ldw,
                        float* bias_grad, void* workspace, size_t workspace_bytes, skf_stream_t stream);
/* the same over live rows (see skf_row_blocks_build): the dgrad form takes a live-ROW list (granule 1) and runs its m
 * tiles over the compacted live rows - rows of A / C / relu_src are gathered through the list, which costs nothing with
 * per-lane load addresses (zero_dead: the dead rows of C are stored as zeros; never when accumulating); the weight
 * gradient contracts over the live 64-row blocks (256 x 256 kernel only; the 128 x 128 kernel visits every row). */
int skf_gemm_bf16_tile_rows(int M, int N, int K, int act);   /* 256 or 128: the m-tile height skf_gemm_bf16 uses for this problem */
int skf_gemm_bf16_rows(int M, int N, int K, const void* A, int lda, const void* B_nk, int ldb, void* C, int ldc,
                       const float* bias, int act, const void* relu_src, int ld_relu, int accumulate, float* C_f32,
                       int ldc_f32, const int* row_list, int zero_dead, skf_stream_t stream);
/* ReLU sign bits of the bf16 path (ffn: builders/layers/transformer.py:196-197): bit (n & 7) of byte [m][n >> 3] (row pitch
 * ld_bits bytes) = "C[m][n] > 0".  A relu forward launch writes them (relu_bits_out), the input-gradient launch of the layer
 * reads them (relu_bits_in) instead of the hidden tensor: same result, 1/16 of the bytes.  N must be a multiple of 8. */
size_t skf_gemm_bf16_relu_bits_bytes(int M, int N);
int skf_gemm_bf16_bits(int M, int N, int K, const void* A, int lda, const void* B_nk, int ldb, void* C, int ldc,
                       const float* bias, int act, const void* relu_src, int ld_relu, int accumulate, float* C_f32, int ldc_f32,
                       const int* row_list, int zero_dead, void* relu_bits_out, const void* relu_bits_in, int ld_bits,
                       skf_stream_t stream);
int skf_gemm_bf16_wgrad_partial_rows(int P, int Q, int R, const void* X, int ldx, const void* dY, int lddy, int splits,
                                     int with_bias_grad, float* slab, size_t slab_bytes, int* splits_used_host,
                                     const int* row_blocks_64, skf_stream_t stream);
int skf_gemm_bf16_wgrad_rows(int P, int Q, int R, const void* X, int ldx, const void* dY, int lddy, float* dW, int ldw,
                             float* bias_grad, void* workspace, size_t workspace_bytes, const int* row_blocks_64,
                             skf_stream_t stream);
/* scaled_dot_product_attention (builders/utils.py:71-105), streaming / online softmax, head size 64, any Lq / Lk;
 * mask semantics and `stats` as skf_attention_fwd.  The backward is two passes (dQ, then dK / dV) and needs
 * skf_attention_bf16_bwd_workspace_bytes of scratch (rowsum(dO o O)).  O_lo (optional, shape and pitch of O): the forward
 * stores the bf16 rounding residual of O there and the backward adds it back when it forms rowsum(dO o O) - that sum is
 * subtracted from dO.V^T, which it nearly cancels where the softmax gradient is small, and 8 significand bits of O leave an
 * error larger than the result in such rows. */
int skf_attention_bf16_fwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const unsigned char* key_mask,
                           int key_mask_ld, int causal, int B, int H, int Lq, int Lk, int dh, void* O, int ldo, void* O_lo,
                           float* stats, skf_stream_t stream);
size_t skf_attention_bf16_bwd_workspace_bytes(int B, int H, int Lq);
int skf_attention_bf16_bwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo,
                           const void* O_lo, const void* dO, int lddo, const float* stats, const unsigned char* key_mask, int key_mask_ld,
                           int causal, int B, int H, int Lq, int Lk, int dh, void* dQ, int lddq, void* dK, int lddk, void* dV,
                           int lddv, void* workspace, size_t workspace_bytes, skf_stream_t stream);
/* the same with per-sample live query counts (skf_target_live_len): query rows >= q_live_len[b] have dO == 0 exactly, so the
 * dQ pass stores zeros for their blocks and the dK / dV pass stops at the last live block */
int skf_attention_bf16_bwd_rows(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo,
                                const void* O_lo, const void* dO, int lddo, const float* stats, const unsigned char* key_mask,
                                int key_mask_ld, int causal, int B, int H, int Lq, int Lk, int dh, void* dQ, int lddq, void* dK,
                                int lddk, void* dV, int lddv, void* workspace, size_t workspace_bytes, const int* q_live_len,
                                skf_stream_t stream);
/* the same with the sorted sample list of skf_sample_order (or NULL): the (sample, head) pairs of the list are dealt over the 8 XCDs and,
 * inside one, over its shader engines (B a multiple of 8, ignored otherwise); a numbering, never a result bit */
int skf_attention_bf16_fwd_ordered(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const unsigned char* key_mask,
                                   int key_mask_ld, int causal, int B, int H, int Lq, int Lk, int dh, void* O, int ldo, void* O_lo,
                                   float* stats, const int* sample_order, skf_stream_t stream);
int skf_attention_bf16_bwd_ordered(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo,
                                   const void* O_lo, const void* dO, int lddo, const float* stats, const unsigned char* key_mask,
                                   int key_mask_ld, int causal, int B, int H, int Lq, int Lk, int dh, void* dQ, int lddq, void* dK,
                                   int lddk, void* dV, int lddv, void* workspace, size_t workspace_bytes, const int* q_live_len,
                                   const int* sample_order, skf_stream_t stream);
/* row kernels: the fp32 entries of the same name with bf16 activations (d in {128, 256, 512, 1024}) */
int skf_embed_fwd_bf16(const long long* tokens, int tok_ld, int B, int L, const float* table, int vocab, int d, const float* pos,
                       void* out, float rate, unsigned site, const void* step_state, skf_stream_t stream);
int skf_embed_bwd_sorted_bf16(const void* ws, int B, int L, const void* dx, int vocab, int d, float* dtable, float rate,
                              unsigned site, const void* step_state, skf_stream_t stream);
int skf_layernorm_residual_fwd_bf16(const void* x, void* y_inout_z, const float* gamma, const float* beta, void* out,
                                    float* stats, int rows, int d, float rate, unsigned site, const void* step_state,
                                    skf_stream_t stream);
size_t skf_layernorm_bwd_bf16_workspace_bytes(int rows, int d);
int skf_layernorm_residual_bwd_bf16(const void* dout, const void* z, const float* stats, const float* gamma, void* dz, void* dy,
                                    float* dgamma, float* dbeta, int rows, int d, float rate, unsigned site,
                                    const void* step_state, void* workspace, size_t workspace_bytes, skf_stream_t stream);
/* rows = B * rows_per_sample; row t of sample b with t >= live_len[b] has dout == 0 exactly: zeros are stored for it */
int skf_layernorm_residual_bwd_bf16_rows(const void* dout, const void* z, const float* stats, const float* gamma, void* dz,
                                         void* dy, float* dgamma, float* dbeta, int rows, int d, float rate, unsigned site,
                                         const void* step_state, void* workspace, size_t workspace_bytes, const int* live_len,
                                         int rows_per_sample, skf_stream_t stream);
/* logits (rows, ld) bf16, even ncls <= ld <= 2048; the gradient is written in place, columns [ncls, ld) as zeros */
int skf_softmax_ce_bf16(void* logits, int ld, int rows, int ncls, const long long* target, int tgt_ld, int tgt_cols, int tgt_off,
                        int mask_pad, float scale, float* row_loss, float* row_hit, int write_grad, skf_stream_t stream);
int skf_pool_fwd_bf16(const void* u, const float* Vw, const void* x, int B, int L, int U, int d, float* a_out, float* emb,
                      skf_stream_t stream);
int skf_pool_bwd_bf16(void* u_inout_dpre, const float* Vw, const void* x, const float* a, const float* demb, int B, int L, int U,
                      int d, void* dx, float* dV, void* workspace, size_t workspace_bytes, skf_stream_t stream);
int skf_expander_fwd_bf16(const float* emb, const float* w, const float* bias, int B, int L, int d, void* pre, skf_stream_t stream);
int skf_expander_bwd_bf16(const void* dpre, const float* emb, const float* w, int B, int L, int d, float* demb,
                          int demb_accumulate, float* dw, float* dbias, void* workspace, size_t workspace_bytes,
                          skf_stream_t stream);
/* fp32 master weight [R][C] (row stride ld_src) -> bf16 images dst [R][ld_dst] and / or dst_t [C][ld_t] (NULL = skip);
 * pad columns are written as zeros.  Plain casts for activations at the fp32 <-> bf16 seams. */
int skf_cast_weight_bf16(const float* src, int R, int C, int ld_src, void* dst, int ld_dst, void* dst_t, int ld_t,
                         skf_stream_t stream);
/* many images in one launch: a DEVICE array of descriptors whose block_begin fields are the running sum of
 * skf_cast_weight_bf16_blocks(R, C, ld_dst, ld_t, &blocks_x) (dst / dst_t may be NULL individually) */
typedef struct SkfCastDesc {
  const float* src; void* dst; void* dst_t;
  int32_t R, C, ld_src, ld_dst, ld_t, block_begin, blocks_x, pad;
} SkfCastDesc;
int skf_cast_weight_bf16_blocks(int R, int C, int ld_dst, int ld_t, int* blocks_x);
int skf_cast_weight_bf16_batch(const SkfCastDesc* descs_dev, int n, int total_blocks, skf_stream_t stream);
int skf_cast_f32_to_bf16(const float* src, void* dst, size_t n, skf_stream_t stream);
int skf_cast_bf16_to_f32(const void* src, float* dst, size_t n, skf_stream_t stream);

/* ------------------------------------------------------------------ the train step
 * Transformer.build_model / call / model_trainer, models/sketchformer.py:63-147, 313-349. */
typedef struct SkfConfig {
  /* sizeof(SkfConfig) as the CALLER compiled / declared it.  skf_config_validate (and with it every entry that takes a
   * config) refuses any other value: a binding that is a field short or long is an error, never a read of heap garbage.
   * skf_config_size() returns the library's figure. */
  uint32_t struct_size;
  /* seq_len <= 512; fp32 path (act_dtype 0) with head size d_model / num_heads = 64: seq_len <= 224, = 32: seq_len <= 448 - what
   * the attention launches hold in LDS (skf_attention_fwd / skf_attention_bwd); skf_config_validate refuses the rest */
  int32_t batch, seq_len, d_model, num_heads, dff, num_layers;
  int32_t vocab_size, n_classes, lowerdim, attn_version;
  int32_t continuous, blind_decoder_mask, max_pos;
  float dropout_rate, recon_weight, class_weight;
  int32_t schedule;
  float sched_p0, sched_p1, sched_p2, sched_p3;
  float beta1, beta2, eps;
  uint32_t seed;
  int32_t use_graph; /* 0: eager launches, weight gradients on a side stream; 1: the step captured into hipGraphs on ONE stream and replayed;
                      * 2: the two-stream step captured (the side stream is forked / joined inside the capture; the first step runs eagerly) -
                      * only with SKF_MODEL_TWO_STREAM_GRAPH set through skf_model_set_flags, otherwise mode 2 issues the same launches
                      * eagerly (bit-equal results): hipGraphLaunch of a multi-branch graph can crash inside the HIP runtime, see the flag.
                      * The default is 0 and is also the fastest */
  int32_t optimizer; /* 0 = Keras Adam (beta1, beta2, eps above), 1 = Keras SGD with momentum (models/sketchformer.py:120-126) */
  float momentum;
  int32_t class_buffer_layers; /* Dense(lowerdim, relu) + Dropout(class_dropout) layers before classify (models/sketchformer.py:44-45,101-104) */
  float class_dropout;
  /* models/sketchformer.py:42,46,76-108: the class head needs lowerdim > 0 and do_classification; the decoder / output
   * layer / expander need do_reconstruction; lowerdim == 0 = no bottleneck, the decoder attends to the encoder output */
  int32_t do_classification, do_reconstruction;
  int32_t gemm_precision; /* SKF_PREC_*: arithmetic of every Dense / attention matmul of the step (0 = fp32 MFMA) */
  /* SKF_ACT_F32 (0): fp32 tensors everywhere (the reference's arithmetic, cfg 1-4).  SKF_ACT_BF16 (1): bf16 activations
   * and weight images, bf16 MFMA with fp32 accumulation, fp32 master weights / Adam (BASELINE cfg 5); token mode with the
   * default structure (attn_version 1, bottleneck + classifier + decoder, no class buffers), head size 64 */
  int32_t act_dtype;
} SkfConfig;
#define SKF_ACT_F32 0
#define SKF_ACT_BF16 1

typedef struct SkfParamEntry {
  char name[96];
  int64_t offset;      /* in floats, into the flat parameter / gradient / moment buffers */
  int32_t rows, cols;  /* logical 2-D shape (1-D variables: rows = 1) */
  int32_t row_stride;  /* floats between rows (fused wq|wk|wv blocks are strided views) */
} SkfParamEntry;

typedef struct SkfModel SkfModel;

size_t skf_config_size(void);                                   /* sizeof(SkfConfig) of this build of the library */
int skf_config_validate(const SkfConfig* cfg);
size_t skf_model_param_floats(const SkfConfig* cfg);            /* length of the flat buffers */
int skf_model_param_entries(const SkfConfig* cfg, SkfParamEntry* out_host, int max_entries); /* returns count */
size_t skf_model_workspace_bytes(const SkfConfig* cfg);

int skf_model_create(const SkfConfig* cfg, SkfModel** out);
void skf_model_destroy(SkfModel* m);
/* Per-model switches (state of THIS model object, not of the library).  SKF_MODEL_DECODE_LAYERWISE: skf_model_greedy_decode
 * runs the layer-by-layer path (one launch per operator, the form the oracle tests pinned first) instead of the one launch
 * per position of skf_decode_fused.hip - same tokens, kept as the cross-check of the fused kernel. */
#define SKF_MODEL_DECODE_LAYERWISE 1u
/* SKF_MODEL_FFN_LAUNCHES: the feed-forward blocks of the step run as separate Dense / LayerNorm launches instead of the one launch
 * per direction of skf_ffn_fused_fwd_f32 / _bwd_f32 (same arithmetic, the sums in a different order): cross-check and A/B. */
#define SKF_MODEL_FFN_LAUNCHES 2u
/* SKF_MODEL_TWO_STREAM_GRAPH: opt-in for SkfConfig.use_graph = 2.  Root cause of the crash recorded in profiles/r05y_two_stream_graph_crash.txt
 * (round 6, from the disassembly of the runtime that ships with torch 2.10+rocm7.0): hip::Graph::UpdateStreams walks the graph exec's internal
 * stream vector WITHOUT a bound while it skips entries that compare equal to the launch stream (the comparison is a virtual call on a
 * member object of the two streams - which object, the binary does not say) - one such entry and it dereferences whatever lies behind
 * the vector.  Which streams compare equal is decided inside the runtime, so a process
 * whose runtime state makes an internal stream of the exec compare equal to the launch stream faults at a replay.  Nothing this library
 * creates or destroys is read on that path.  tools/micro/graph_parallel_stream_alias.hip tries to provoke it with plain HIP calls
 * (stream counts, build / replay / destroy cycles, leaked execs, stream 0): none of its 72 cases faults (profiles/r06b_graph_alias.txt) -
 * the trigger needs the history of the process that showed it (pytest over two test files) and was not isolated.  Set the flag only in
 * a process of its own (the test and bench.py use a child process). */
#define SKF_MODEL_TWO_STREAM_GRAPH 4u
int skf_model_set_flags(SkfModel* m, uint32_t flags);
/* params/grads/adam_m/adam_v: skf_model_param_floats floats each; pos: (max_pos, d_model) table
 * (builders/utils.py:17-32, computed by the host in float64 like the reference);
 * metrics: 32 floats; step_state: skf_step_state_bytes bytes.  All device memory owned by the caller. */
int skf_model_bind(SkfModel* m, float* params, float* grads, float* adam_m, float* adam_v, const float* pos,
                   void* workspace, size_t workspace_bytes, float* metrics, void* step_state);
/* forward only (Transformer.call); training != 0 enables dropout.  inp/tar: (B,L) int64 tokens, or (B,L,5) float32
 * stroke-5 rows when cfg.continuous; tar has row stride tar_ld (in sequence positions), its first L-1 positions feed the decoder. */
int skf_model_forward(SkfModel* m, const void* inp, const void* tar, int tar_ld, int training,
                      skf_stream_t stream);
/* Every call that takes inp / tar / labels copies them into the model's workspace first (one launch on `stream`) and records the model's
 * "inputs staged" event behind that copy.  A caller that passes DEVICE tensors which it will overwrite for the next batch makes the
 * stream that overwrites them wait here - the step itself is not waited for, and nothing has to be cloned in front of the call. */
int skf_model_wait_inputs_staged(SkfModel* m, skf_stream_t stream);
/* model_trainer minus apply_gradients: forward, losses, metrics, backward into `grads`. labels (B,1) int64. */
int skf_model_forward_backward(SkfModel* m, const void* inp, const void* tar, int tar_ld,
                               const long long* labels, skf_stream_t stream);
/* optimizer.apply_gradients with grads pre-multiplied by grad_scale (1/world_size under data parallelism) */
int skf_model_apply_gradients(SkfModel* m, float grad_scale, skf_stream_t stream);
/* ---- data-parallel hooks: the flat gradient buffer becomes final in pieces ("buckets", in production order:
 * [decoder embedding .. output layer] after the decoder backward, then [encoder .. expander]).  A caller that
 * all-reduces gradients makes its communication stream wait for a bucket, reduces that slice of `grads`, and applies the
 * optimizer per slice - the all-reduce of bucket 0 overlaps the encoder backward, that of bucket 1 the optimizer sweep of
 * bucket 0.  skf_model_grad_buckets returns the number of buckets (1 when the step is replayed from hipGraphs);
 * offsets/counts in floats.  skf_model_apply_gradients_range == skf_model_apply_gradients on one slice
 * (last != 0: also ends the step, iterations += 1). */
int skf_model_grad_buckets(SkfModel* m, int max_buckets, size_t* offsets_host, size_t* counts_host);
int skf_model_wait_grad_bucket(SkfModel* m, int bucket, skf_stream_t stream);
int skf_model_apply_gradients_range(SkfModel* m, size_t offset, size_t count, float grad_scale, int last,
                                    skf_stream_t stream);

/* ------------------------------------------------------------------ gradient norms and clipping (skf_gradnorm.hip)
 * tf.keras optimizers' clipnorm / global_clipnorm / clipvalue, a gradient-norm read-out and a guard against non-finite gradients,
 * over ANY flat fp32 buffer described by SkfParamEntry rows (name unused; offset, rows, cols, row_stride as in the model's table:
 * strided views are read as such, floats between entries are never read).  Everything the step decides is decided on the device.
 *
 * Segment plan: the host cuts every entry into chunks of SKF_SEGMENT_CHUNK logical elements (row-major; the last chunk of an entry
 *   is ragged) - a constant, so no result depends on the grid or the device.  skf_segment_plan_chunks -> the chunk count (negative:
 *   error); skf_segment_plan_build fills skf_segment_plan_bytes(n_entries, n_chunks) bytes of HOST memory, which the caller copies
 *   to the device (16-byte aligned) once per layout.  Limits (SKF_EINVAL): offset >= 0, rows, cols >= 1, row_stride >= cols,
 *   rows * cols < 2^31 - SKF_SEGMENT_CHUNK.
 * skf_segment_norms: two launches.  (1) one workgroup per chunk: fp64 sum of squares (16-byte loads where offset, cols and
 *   row_stride are multiples of 4 floats or the entry is contiguous; scalar loads otherwise and for tails) and the count of
 *   non-finite elements, reduced in a fixed order, no atomics.  (2) one workgroup folds the partials of an entry in chunk order and
 *   the entries in table order and writes `stats`, skf_segment_stats_floats(E) = 8 + 2 E 4-byte words:
 *     [0] f32 global norm = (float)(sqrt(sum) * grad_scale)   [1] f32 applied global scale   [2] u32 non-finite elements
 *     [3] u32 skip flag = skip_nonfinite && [2] != 0          [4] u32 skipped total (ONLY the clipped sweeps add to it; zero it once)
 *     [5..7] reserved   [8 .. 8+E) f32 per-entry norms   [8+E .. 8+2E) f32 per-entry scales
 *   grad_scale is a factor on the norms (1/world_size under data parallelism); the buffer itself is not rescaled.
 *   Scales, fp32, each operation rounded once: SKF_CLIP_GLOBAL  [1] = c / max(norm, c), entry scales 1;
 *   SKF_CLIP_PER_VARIABLE  s_e = c / max(norm_e, c), [1] = 1; SKF_CLIP_NONE  all 1 (norms only).  norm <= c gives exactly 1.
 *   workspace: skf_segment_norms_workspace_bytes(E, n_chunks), 256-byte aligned.  SKF_EINVAL: threshold <= 0 or non-finite in a norm mode.
 * skf_segment_scale: one launch over the plan, every element of entry e times scales[e] in place; skip != NULL and *skip != 0:
 *   nothing is written.
 * skf_gradient_clip_validate: the rule of the settings (host only): at most one of {per-variable, global, clipvalue > 0}; the
 *   threshold of a norm mode and a clipvalue finite and > 0 (clipvalue 0 = off). */
#define SKF_SEGMENT_CHUNK 16384
#define SKF_CLIP_NONE 0
#define SKF_CLIP_PER_VARIABLE 1
#define SKF_CLIP_GLOBAL 2
int skf_segment_plan_chunks(const SkfParamEntry* entries_host, int n_entries);
size_t skf_segment_plan_bytes(int n_entries, int n_chunks);
int skf_segment_plan_build(const SkfParamEntry* entries_host, int n_entries, void* plan_host, size_t plan_bytes);
size_t skf_segment_norms_workspace_bytes(int n_entries, int n_chunks);
size_t skf_segment_stats_floats(int n_entries);
int skf_gradient_clip_validate(int mode, float threshold, float clipvalue);
int skf_segment_norms(const float* flat, const void* plan_dev, int n_entries, int n_chunks, float grad_scale, int mode,
                      float threshold, int skip_nonfinite, void* workspace, size_t workspace_bytes, float* stats,
                      skf_stream_t stream);
int skf_segment_scale(float* flat, const void* plan_dev, int n_entries, int n_chunks, const float* scales, const void* skip,
                      skf_stream_t stream);
/* The sweeps with device-side control: skf_adam_step / skf_sgd_momentum_step on the gradient
 *   gg = (g * grad_scale) * s;  clipvalue > 0: gg = min(max(gg, -clipvalue), clipvalue)
 * s = *scale (device float; NULL = 1), every product rounded on its own: the update equals the plain sweep over a gradient scaled /
 * clamped in memory bit for bit.  skip (NULL = never): two device words {flag, total}, e.g. stats + 3: with the flag set the sweep
 * writes nothing, `iterations` is not advanced and the total goes up by one.  advance != 0: the sweep also closes the step
 * (iterations += 1, what skf_step_epilogue does) unless it is skipped. */
int skf_adam_step_clipped(float* w, const float* g, float* m, float* v, size_t n, void* step_state, float grad_scale,
                          const float* scale, float clipvalue, void* skip, float beta1, float beta2, float eps, int advance,
                          skf_stream_t stream);
int skf_sgd_momentum_step_clipped(float* w, const float* g, float* velocity, size_t n, void* step_state, float grad_scale,
                                  const float* scale, float clipvalue, void* skip, float momentum, int advance,
                                  skf_stream_t stream);
/* The train step with the above.  skf_model_set_gradient_clip configures THIS model: mode / threshold / clipvalue as in
 * skf_gradient_clip_validate (SKF_EINVAL with a message otherwise), skip_nonfinite: a step whose gradient holds an inf or NaN changes
 * nothing (parameters, moments, iterations) and counts as skipped; monitor: compute the norms even when nothing else needs them.
 * workspace: skf_model_clip_workspace_bytes(cfg) bytes of caller-owned device memory, 256-byte aligned, which starts with the stats
 * words of skf_segment_norms for the model's entry table (skf_model_param_entries order) - read them from there, no call needed; the
 * call uploads the segment plan behind them and zeroes the stats (it synchronises the device: a step in flight may read the old
 * settings).  Mode none, clipvalue 0, skip_nonfinite 0 and monitor 0 switch everything off again (workspace may be NULL).
 * skf_model_apply_gradients_clipped: skf_model_apply_gradients for a configured model (SKF_EINVAL for an unconfigured one): the two
 * norm launches (not with clipvalue alone), the segment scale in per-variable mode, then ONE clipped sweep that also closes the step -
 * a constant launch sequence with no host synchronisation; under use_graph it is captured once and re-captured when grad_scale or
 * a setting changes.  skf_model_apply_gradients / _range never clip. */
size_t skf_model_clip_workspace_bytes(const SkfConfig* cfg);
int skf_model_set_gradient_clip(SkfModel* m, int mode, float threshold, float clipvalue, int skip_nonfinite, int monitor,
                                void* workspace, size_t workspace_bytes);
int skf_model_apply_gradients_clipped(SkfModel* m, float grad_scale, skf_stream_t stream);
/* Gradient accumulation in the train step: k micro-batches, one optimizer step.  acc: skf_model_param_floats floats of caller-owned
 * device memory, 16-byte aligned.  After every skf_model_forward_backward (which overwrites `grads`) the caller issues one phase on
 * the stream the step ran on (backward leaves `grads` complete there):
 *   SKF_ACCUM_FIRST  acc = grads          micro += 1     the first micro-batch of an optimizer step (acc's old contents are dropped)
 *   SKF_ACCUM_ADD    acc += grads         micro += 1     micro-batches 2 .. k-1
 *   SKF_ACCUM_CLOSE  grads = acc + grads  micro  = 0     the last one: `grads` holds the SUM of the k micro-batch gradients
 *   SKF_ACCUM_RESET  nothing              micro  = 0     drop what is pending
 * and after CLOSE the unchanged skf_model_apply_gradients[_clipped | _range] with grad_scale = 1 / (world_size * k): the sweep,
 * the norms, the clip scale, the skip rule and iterations += 1 then act on the mean gradient.  A non-finite micro-gradient poisons
 * the sum: with skip_nonfinite the whole accumulated step is skipped and counted once; `micro` is already 0 by then, so the next
 * step starts clean either way.  Each phase is ONE launch (skf_grad_accumulate), no host synchronisation, and is issued eagerly
 * also under use_graph (its operands would make one captured graph per phase and buffer; the captured step graphs on either side
 * read `micro` and `grads` from device memory and replay unchanged).  A model that never calls this runs the step it always ran. */
#define SKF_ACCUM_FIRST 0
#define SKF_ACCUM_ADD 1
#define SKF_ACCUM_CLOSE 2
#define SKF_ACCUM_RESET 3
int skf_model_accumulate_gradients(SkfModel* m, float* acc, int phase, skf_stream_t stream);
/* Weight averaging in the train step: an exponential moving average of `params` that evaluation and sampling run on.
 * skf_model_set_weight_average: shadow = skf_model_param_floats floats of caller-owned device memory, 16-byte aligned (NULL = off);
 *   decay in (0, 1); num_updates != 0 = the warm-up rule min(decay, (1 + n) / (10 + n)) over n = iterations.  It does NOT initialise
 *   the shadow: tf starts a shadow at the variable's value, so copy `params` into it.
 * skf_model_update_weight_average: ONE eager launch (skf_ema_update) on the stream the step ran on, issued behind
 *   skf_model_apply_gradients, skf_model_apply_gradients_clipped or the last skf_model_apply_gradients_range: the sweep has advanced
 *   `iterations` by then, so n is the number of updates applied (tfa: num_updates = optimizer.iterations).  With a clip configuration
 *   that computes norms it reads the sweep's skip flag: a skipped step leaves the shadow untouched, as it leaves parameters, moments
 *   and `iterations` untouched.  Under gradient accumulation: once per optimizer step.  It is not part of the captured step graphs:
 *   under use_graph it follows the replay, as the accumulate phases do.
 * skf_model_swap_weight_average: params <-> shadow in place (skf_buffer_swap), toggles "average live".  Every forward rebuilds its
 *   weight images from `params`, so every inference entry then runs on the average.  While the average is live
 *   skf_model_forward_backward, the three apply_gradients entries, skf_model_accumulate_gradients and
 *   skf_model_update_weight_average return SKF_EINVAL with a message (one host branch on a flag no other model ever sets).
 * skf_model_weight_average_live: 1 while live, else 0.  A model that never calls these runs the step it always ran. */
int skf_model_set_weight_average(SkfModel* m, float* shadow, float decay, int num_updates);
int skf_model_update_weight_average(SkfModel* m, skf_stream_t stream);
int skf_model_swap_weight_average(SkfModel* m, skf_stream_t stream);
int skf_model_weight_average_live(SkfModel* m);
/* ---- inference API of the plugin (models/sketchformer.py:162-168, 201-311) ----
 * skf_model_encode: encode_from_seq / predict_class - encoder + bottleneck + classifier with dropout off; results in
 *   the buffers "embedding" (B,d), "class_probs" (B,C), "enc_output" (B*L,d).
 * skf_model_greedy_decode: predict_from_embedding - greedy reconstruction with a per-layer K/V cache.
 *   embedding: (B,d) device floats, or NULL to use the model's own "embedding" buffer (after skf_model_encode);
 *   expected_len_host: per-sample key limit of the cross attention, used only when blind_decoder_mask == 0 (NULL = i+1);
 *   only the first n_valid samples take part in the stop test; sos/eos: tokenizer ids (ignored in continuous mode);
 *   out: device buffer (B, max_steps+1) int64 tokens [column 0 = SOS] or (B, max_steps+1, 5) float stroke-5 rows
 *   [row 0 = (0,0,1,0,0)]; *out_len_host = number of valid columns (the reference's output length).
 *   Blocking: synchronises the stream every 8 tokens to test the stop condition. */
/* skf_model_greedy_decode_attn: the same, plus the decoder's attention weights (models/sketchformer.py:204,220,306
 *   out['attn_weights'] = the Decoder's dict decoder_layer{i}_block1 / _block2, builders/layers/transformer.py:245-262,328-344).
 *   attn_weights: NULL (= skf_model_greedy_decode), or a device buffer of (2 * num_layers, B, H, max_steps, seq_len) floats:
 *   index 2l = layer l's block1 (self attention), 2l + 1 its block2 (cross attention over pre_decoder); row t of (b, h) = the
 *   softmax row of position t (builders/utils.py:101-105), block1 zero from key t + 1 on.  Every row of a decoded position is
 *   written in full (no memset needed); rows of positions not decoded are left as they were.
 *   With T = *out_len_host - 1, rows [0, T) of a block are what the reference's last decoder pass returns over recon[:, :T]:
 *   block1[..., :T, :T] (look-ahead | target padding mask), block2[..., :T, :] (keys >= expected_len masked unless blind;
 *   masked entries exactly 0).  Capturing during the KV-cached decode is exact because both masks stay the same from step
 *   to step - except with blind_decoder_mask == 0 and expected_len_host == NULL (nattn = i + 1 changes every iteration):
 *   that combination is refused (SKF_EINVAL).  The weights-off path is unchanged (captured step, one launch per position). */
int skf_model_encode(SkfModel* m, const void* inp, skf_stream_t stream);
int skf_model_greedy_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid,
                            long long sos, long long eos, int max_steps, void* out, int* out_len_host,
                            skf_stream_t stream);
int skf_model_greedy_decode_attn(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid,
                                 long long sos, long long eos, int max_steps, void* out, int* out_len_host,
                                 float* attn_weights, skf_stream_t stream);
/* skf_model_sample_decode: skf_model_greedy_decode with every token DRAWN by the selection rule above (skf_decode_sample_tokens)
 *   instead of maximised: position i of row b uses u = skf_sample_uniform(sampling->seed, stream_id[b], i).
 *   stream_ids_host: B host ints, NULL = 0 .. B-1.  Same outputs, stop rule and blocking behaviour as the greedy entry; one launch
 *   per position (the sampling instantiation of the same kernel), or with SKF_MODEL_DECODE_LAYERWISE the layer-by-layer steps
 *   issued eagerly.  Keeps no state: greedy decoding before and after is unchanged.
 *   Continuous models are refused (SKF_EUNSUPPORTED): there is no categorical head to draw from. */
int skf_model_sample_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid,
                            long long sos, long long eos, int max_steps, void* out, int* out_len_host,
                            const SkfSampling* sampling, const int* stream_ids_host, skf_stream_t stream);
/* skf_model_beam_decode: beam-search reconstruction (the rule above) of n = batch / beam_width sketches, token models only.
 *   embedding: (n, E) device floats [(n, L, d) without a bottleneck], required; it is replicated into the W rows of every sketch on
 *   the device, and so is expected_len_host (n host ints; required when blind_decoder_mask == 0).  Only the first n_valid <= n
 *   sketches take part in the stop test: the decode ends at the first position after which every one of their beams is finished.
 *   out_tokens (n, W, max_steps + 1) int64 [column 0 = SOS, zeros from *out_len_host on], out_scores (n, W) the raw fp32 sums of
 *   log p, out_lengths (n, W): device buffers, the hypotheses of a sketch ordered by score / ((5 + len) / 6)^length_alpha
 *   descending, then beam index ascending.  A finished hypothesis carries PADs behind its EOS and keeps its score.
 *   Always one position launch + one advance launch per position: SKF_MODEL_DECODE_LAYERWISE does not affect it (there are no beams
 *   on the layer-by-layer path).  Blocking like the greedy entry (stop test every 8 positions).  Keeps no state.
 *   SKF_EINVAL: a continuous model (its output is one deterministic row, nothing to rank); beam_width outside
 *   [1, min(8, vocab_size, batch)]; length_alpha < 0 or not finite; a model the one-launch beam kernel does not serve; a non-blind
 *   model without expected_len_host; n_valid outside [1, n].
 *   The buffers "decode/tokens" (B, 2 (L + 1)) [int64 image seen as floats] and "decode/ancestry" (B, L + 1) [ints] hold the running
 *   image and the ancestry table the hypotheses of the last call were gathered through.  They are diagnostics (the tests re-read
 *   the hypotheses through them) and NOT part of the stable interface: names, shapes and element views may change. */
int skf_model_beam_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                          long long eos, int max_steps, long long* out_tokens, float* out_scores, int* out_lengths,
                          int* out_len_host, const SkfBeam* beam, skf_stream_t stream);
/* ---- sketch completion: prefix-forced decoding ----
 * The rule.  A prefix gives row b a length len[b], 0 <= len[b] <= max_steps, and tokens prefix[b][0 .. len[b]-1]; they become the
 * output columns 1 .. len[b].  Position s is the step that reads column s and writes column s + 1; it is FORCED for row b iff
 * s < len[b].  A forced position writes prefix[b][s] to column s + 1 with every effect an emitted token has (the mask byte
 * token == 0, the sticky EOS flag, its part in the stop test), appends the position's K|V row to every layer's cache, and computes no
 * logits.  A token outside [0, vocab) is treated as PAD, as the embedding lookup does.
 *   Sampling: u = skf_sample_uniform(seed, stream_id[b], position) is a function of the absolute position: a forced position
 *   consumes nothing and shifts nothing.
 *   Beam search: at a forced position a live beam offers exactly one candidate, (0.0f, prefix token); its other offers are -inf.  The
 *   merge (skf_beam_advance) is what it was, so the returned scores are log p(continuation | prefix, embedding).  The prefix and the
 *   length of sketch g are replicated into the W rows of the sketch on the device, like the embedding.
 *   Stop rule: unchanged, and a forced EOS counts.  If every one of the n_valid rows has an EOS inside its prefix the decode ends
 *   inside the prefix, and *out_len_host is what stepping through it reports.
 *   len = 0 everywhere is exactly skf_model_greedy_decode / _sample_decode / _beam_decode.
 * SkfPrefix: tokens (rows, ld) int64 on the device, len_host `rows` host ints; rows = batch for skf_model_prefix_decode, n = batch /
 *   beam_width for skf_model_beam_prefix_decode.  stepwise = 0: the cache rows of all forced positions are produced first, layer by
 *   layer, in num_layers launches over (max len, rows) workgroups (the prefill), and the position loop starts at the shortest
 *   prefix; rows with a longer one idle through their remaining forced positions.  stepwise = 1: every forced position is one
 *   position launch, like a free one.  Both give the same bits: outputs, lengths and cache rows.  The beam entry always steps.
 * skf_model_prefix_decode: skf_model_greedy_decode (sampling == NULL) or skf_model_sample_decode (sampling, stream_ids_host) with
 *   a prefix.  skf_model_beam_prefix_decode: skf_model_beam_decode with one.
 *   SKF_EINVAL: prefix == NULL, a bad struct_size, a null tokens / len_host, a length outside [0, max_steps], ld < the largest length,
 *   and whatever the entry without a prefix refuses.  SKF_EUNSUPPORTED: a continuous model; SKF_MODEL_DECODE_LAYERWISE, or dimensions
 *   the one-launch position kernel does not serve (prefixes exist on that kernel only).
 *   The buffers "decode/cache0" .. "decode/cache{N-1}" (B * L, 2 d) hold the self-attention K|V rows of the last reconstruction; like
 *   "decode/tokens" they are diagnostics and NOT part of the stable interface. */
typedef struct SkfPrefix {
  uint32_t struct_size;    /* sizeof(SkfPrefix) */
  const long long* tokens; /* device (rows, ld) */
  int32_t ld;
  const int* len_host;     /* rows host ints, 0 <= len <= max_steps */
  int32_t stepwise;        /* 0: prefill + skip; 1: step through the forced positions */
} SkfPrefix;
int skf_model_prefix_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                            long long eos, int max_steps, void* out, int* out_len_host, const SkfPrefix* prefix,
                            const SkfSampling* sampling, const int* stream_ids_host, skf_stream_t stream);
int skf_model_beam_prefix_decode(SkfModel* m, const float* embedding, const int* expected_len_host, int n_valid, long long sos,
                                 long long eos, int max_steps, long long* out_tokens, float* out_scores, int* out_lengths,
                                 int* out_len_host, const SkfBeam* beam, const SkfPrefix* prefix, skf_stream_t stream);
/* look up an internal activation by name ("logits", "class_probs", "embedding", "enc_output", ...); skf_model_buffer serves
 * fp32 buffers, skf_model_buffer_info any buffer with its row pitch (elements) and element type (bf16 models keep their
 * activations in bf16) */
int skf_model_buffer_info(SkfModel* m, const char* name, void** ptr, int* rows, int* cols, int* ld, int* is_bf16);
int skf_model_buffer(SkfModel* m, const char* name, float** ptr, int* rows, int* cols);

/* ------------------------------------------------------------------ Retrieval
 * The third task the reference's README names for the learned embedding (classification, reconstruction / interpolation,
 * image retrieval); the reference ships no code for it.  Serves the (N, d) embeddings that models/sketchformer.py:162-168
 * (predict_class) returns and experiments/extract_embeddings.py writes.
 * skf_knn_topk_f32: for each of Q query rows the k gallery rows with the smallest squared Euclidean distance
 *   |q|^2 + |g|^2 - 2 q.g, ascending: out_idx (Q, k) int32 gallery rows, out_dist (Q, k) fp32.  Exact search: the Q x G scores
 *   are formed tile by tile on the fp32 matrix cores and never stored.  Equal distances come out in gallery-row order; the
 *   distance of a (query, gallery row) pair does not depend on where either row sits, nor on how the search was cut up, so two
 *   calls over the same rows agree bit for bit.  exclude (NULL, or Q int32, -1 = none): one gallery row per query that is left
 *   out of its ranking (leave-one-out over a single split: exclude[i] = i).
 *   Limits (SKF_EINVAL): d % 4 == 0, 4 <= d <= 1024, 1 <= k <= 128, k <= G (G - 1 with exclude), Q >= 1, rows 16-byte aligned
 *   (base pointers and ldq, ldg % 4 == 0).  Inputs must be finite.  workspace: skf_knn_workspace_bytes(Q, G, k) bytes
 *   (0 = bad sizes), 16-byte aligned.
 * skf_row_normalize_f32: y = x / max(|x|, 1e-12) per row, out of place.  The cosine ranking is the same search on normalised
 *   rows; the distance reported is then 2 - 2 cos. */
size_t skf_knn_workspace_bytes(int Q, int G, int k);
int skf_knn_topk_f32(const float* queries, int ldq, int Q, const float* gallery, int ldg, int G, int d, int k,
                     const int* exclude, int* out_idx, float* out_dist, void* workspace, size_t workspace_bytes,
                     skf_stream_t stream);
int skf_row_normalize_f32(const float* x, int ldx, int rows, int d, float* y, int ldy, skf_stream_t stream);

/* ------------------------------------------------------------------ Token dictionary (k-means)
 * The dictionary of the default tokenizer: prep_data/sketch_token/create_token_dict.py:104-109 fits sklearn KMeans(n_clusters=1000,
 * n_init=10, max_iter=500, tol=1e-6) over 5 M normalised (dx, dy) offsets, and utils/tokenizer.py:43 maps every offset to its
 * nearest centre (KMeans.predict).  Lloyd iterations for 2-D points:
 * skf_kmeans_assign_f32: labels[i] (N int32) = the nearest of K centres for point i, and optionally dist[i] (N fp32, NULL = not
 *   wanted) = its squared distance.  The distance of a pair is DEFINED as dx = x - cx; dy = y - cy; fmaf(dy, dy, dx * dx) in fp32,
 *   so it depends on the two rows alone; among equal minima the lowest centre index wins (the first-minimum rule of argmin).
 * skf_kmeans_step_f32: one Lloyd iteration, always the same three commands (clear accumulators, assign + accumulate, update):
 *   labels as above against the centres going in; per centre the count (counts, K int32, NULL = not wanted) and the mean of its
 *   points, written over `centers` in place - a centre that received no point keeps its coordinates; into *state the inertia (sum
 *   of the minimum distances, fp64), the squared shift sum |c_new - c_old|^2 (fp64), the number of empty centres, and
 *   iterations += 1.  Coordinates are accumulated as 64-bit integers of rint(x * 2^scale_exp) - the caller picks scale_exp once per
 *   fit so that max|coordinate| * 2^scale_exp < 2^30 - and the mean is formed in fp64 and rounded once to fp32, the inertia is
 *   summed in a fixed order: the result is bit-identical from run to run and does not depend on grid size or arrival order.
 *   Stop flag: when shift <= tol_abs the update sets state->converged; every later step on that state returns at once and leaves
 *   centres, labels, counts and state as that iteration wrote them (tol_abs < 0: never stops).  A fit zeroes the state block
 *   once, enqueues steps in groups and reads the block once per group; nothing here synchronises with the host.
 *   Limits: d == 2 (else SKF_EUNSUPPORTED); SKF_EINVAL: 1 <= K <= 4096, 1 <= N < 2^31, rows 8-byte aligned (base pointers, and ldp,
 *   ldc even), scale_exp in [-126, 127].  Inputs must be finite.  workspace: skf_kmeans_workspace_bytes(N, K) bytes (0 = bad
 *   sizes), 16-byte aligned; its contents carry nothing from one step to the next. */
typedef struct SkfKmeansState {
  int32_t iterations; /* Lloyd iterations performed on this state */
  int32_t converged;  /* set by the iteration whose shift <= tol_abs */
  int32_t n_empty;    /* centres that received no point in the last iteration */
  int32_t pad;
  double inertia;     /* of the last iteration's assignment */
  double shift;       /* sum |c_new - c_old|^2 of the last iteration */
} SkfKmeansState;
size_t skf_kmeans_workspace_bytes(long long N, int K);
int skf_kmeans_assign_f32(const float* points, int ldp, long long N, int d, const float* centers, int ldc, int K,
                          int* labels, float* dist, skf_stream_t stream);
int skf_kmeans_step_f32(const float* points, int ldp, long long N, int d, float* centers, int ldc, int K, int scale_exp,
                        double tol_abs, int* labels, int* counts, SkfKmeansState* state, void* workspace,
                        size_t workspace_bytes, skf_stream_t stream);

/* ------------------------------------------------------------------ Latent interpolation
 * The step between encode and greedy decode of experiments/interpolations_for_mturk.py:98-108: utils/skt_tools.py:18-25 (slerp) and
 * :28-30 (lerp), for P pairs and T steps in one launch.
 * skf_interpolate_f32: a, b (P, d) fp32 rows, t T fp32 steps, all on the device; out (P * T, d): row p * T + j is the
 *   interpolation of (a[p], b[p]) at t[j].  mode 0 = slerp, 1 = lerp.
 *   slerp: per pair aa = sum a_i^2, bb = sum b_i^2, ab = sum a_i b_i in fp64 (the products are exact; the three sums run over the
 *   same elements in the same order), c = ab / sqrt(aa * bb) CLAMPED to [-1, 1], omega = acos(c), so = sin(omega), all fp64.  The
 *   reference takes arccos of the unclamped dot product and returns NaN once rounding pushes |c| past 1; here those pairs take the
 *   next branch.  so < 1e-6 (same or opposite direction, the reference's `return p0`): every row of the pair is a copy of a[p].
 *   Otherwise w0 = (float)(sin((1 - (double)t_j) * omega) / so), w1 = (float)(sin((double)t_j * omega) / so).
 *   lerp: w0 = 1.0f - t_j, w1 = t_j.  Elements, both modes, fp32: out_i = fmaf(w1, b_i, w0 * a_i).  So t = 0 gives the row a[p] and
 *   t = 1 the row b[p], exactly; b = s a with s a power of two gives c = 1 exactly; two calls on the same inputs agree bit for bit.
 *   Limits (SKF_EINVAL): d % 4 == 0, 4 <= d <= 4096, 1 <= T <= 256, P >= 1, P * T < 2^31, rows 16-byte aligned (base pointers of
 *   a, b, out and lda, ldb, ldo % 4 == 0, each >= d), mode in {0, 1}.  Columns >= d of out are left alone.  out must not alias a
 *   or b (not checked).  Inputs must be finite with non-zero norm. */
int skf_interpolate_f32(const float* a, int lda, const float* b, int ldb, int P, int d, const float* t, int T, int mode,
                        float* out, int ldo, skf_stream_t stream);

/* ------------------------------------------------------------------ Embedding map (exact t-SNE)
 * The t-SNE map of the evaluation (metrics/visualisation.py of the reference asks sklearn.manifold.TSNE for it): the exact O(N^2)
 * algorithm of van der Maaten & Hinton (2008) with the semantics of scikit-learn's method='exact', no Barnes-Hut.  Nothing here
 * allocates or synchronises with the host; every sum has a fixed order (no floating-point atomic), so two calls on the same
 * inputs agree bit for bit.  workspace: skf_tsne_workspace_bytes(N) bytes (0 = bad N), 16-byte aligned; its contents carry nothing
 * from one call to the next.
 * skf_tsne_affinities_f32: x (N, d) fp32 -> the joint probabilities P (N, N) fp32 and, when beta != NULL, the N precisions (fp64).
 *   The distance of a pair is DEFINED as D_ij = sum_k (x_ik - x_jk)^2 in fp32, acc = fmaf(diff, diff, acc) over k ascending from
 *   acc = 0: direct differences, so D_ii == 0 and D_ij == D_ji bit for bit.  Row i is searched over j != i with
 *   e_j = (double)D_ij - (double)min_{j != i} D_ij, p_j = exp(-beta e_j), S = sum p_j, H = log S + beta sum e_j p_j / S, all fp64:
 *   beta starts at 1 with bounds (0, inf); 64 evaluations, none skipped; after each, H > log(perplexity) makes beta the lower bound
 *   and doubles it while no upper bound exists, else moves it to the middle of the bounds; otherwise beta becomes the upper bound
 *   and moves to the middle.  beta_i and S_i are those of the 64th evaluation.  Entries with D_ij == 0 (duplicates of row i) are
 *   counted into S as exact ones instead of being added in place, so identical rows of x get identical beta and S.  The sign of
 *   H - log(perplexity) is taken from that expression while S <= 0.75 n (n = N - 1), and above it - a row near uniformity, where
 *   log S and beta sum e p / S cancel - from the identical log(n / perplexity) - (1 / n) sum_j f(x_j), f(x) = (1 + x) log(1 + x) - x,
 *   x_j = n p_j / S - 1 = (expm1(-beta e_j) - m) / (1 + m), m = mean_j expm1(-beta e_j): every term is non-negative, so the sign
 *   is exact down to beta = 2^-63 (perplexity = N - 1 ends there) instead of following rounding noise.  The conditional
 *   is p_{j|i} = exp(-beta_i e_j) / S_i in fp64 and P_ij = (float)((p_{j|i} + p_{i|j}) / (2 N)): P_ii == 0, P_ij == P_ji bit for bit.
 *   Limits (SKF_EINVAL): 3 <= N <= 8192, 4 <= d <= 1024, d % 4 == 0, 1 <= perplexity <= N - 1, rows of x and P 16-byte aligned
 *   (base pointers, ldx % 4 == 0, ldp % 4 == 0, ldx >= d, ldp >= N).  Columns >= N of P are left alone.  Inputs must be finite.
 * skf_tsne_step_f32: one gradient-descent iteration, two launches, in place on Y, U (velocity) and gains, contiguous (N, 2) fp32.
 *   Pair pass: q_ij is DEFINED as dx = y_i0 - y_j0; dy = y_i1 - y_j1; q = rcp(1 + fmaf(dy, dy, dx * dx)) in fp32 (rcp: the
 *   hardware reciprocal, 1 ulp); per row, in fp32, z_i = sum_{j != i} q_ij, a_i = sum_j P_ij q_ij (y_i - y_j),
 *   r_i = sum_j q_ij^2 (y_i - y_j).  Update: Z = sum_i z_i in fp64 (no second pass over the pairs) and
 *   g = (float)(4 (exaggeration a_i - r_i / Z)) in fp64 from the fp32 row sums; grad (N, 2), if not NULL, receives g.  Then, every
 *   operation rounded to fp32 on its own (no fused multiply-add): gain' = (U * g < 0) ? gain + 0.2f : gain * 0.8f;
 *   gain' = max(gain', 0.01f); U' = momentum * U - learning_rate * (gain' * g); Y' = Y + U'.  No recentring.
 * skf_tsne_kl_f32: *kl_out (a device double) = sum over P_ij > 0 of P_ij log(P_ij / Q_ij), Q_ij = q_ij / Z, with q and z_i as
 *   above (fp32) and everything else in fp64, as sum_ij P_ij log(P_ij / q_ij) + log Z sum_ij P_ij.
 *   Limits of both (SKF_EINVAL): 3 <= N <= 8192, rows of P 16-byte aligned, the (N, 2) arrays 8-byte aligned. */
size_t skf_tsne_workspace_bytes(int N);
int skf_tsne_affinities_f32(const float* x, int ldx, int N, int d, double perplexity, float* P, int ldp, double* beta,
                            void* workspace, size_t workspace_bytes, skf_stream_t stream);
int skf_tsne_step_f32(const float* P, int ldp, int N, float* Y, float* U, float* gains, float* grad, float exaggeration,
                      float momentum, float learning_rate, void* workspace, size_t workspace_bytes, skf_stream_t stream);
int skf_tsne_kl_f32(const float* P, int ldp, int N, const float* Y, double* kl_out, void* workspace, size_t workspace_bytes,
                    skf_stream_t stream);

/* ------------------------------------------------------------------ Sketches as images (rasterizer, overlap score)
 * The reference draws sketches through utils/sketch.py (svgwrite -> svglib); here a sketch becomes a coverage image on the device,
 * so that a reconstruction can be laid over its original and scored.  Nothing here allocates, synchronises with the host or uses
 * an atomic; two calls on the same inputs agree bit for bit and a sketch's results do not depend on the rest of the batch.
 * skf_sketch_points: B sketches of at most T positions -> drawable points.  kind selects the encoding of `data`; the project's
 *   host decoders are the specification:
 *     SKF_SKETCH_STROKE3: fp32 rows (dx, dy, pen), ld floats from sketch to sketch (>= 3 T); lengths[b] rows are used (clamped to
 *       [0, T]); every row is a point, its pen is lifted where pen == 1.
 *     SKF_SKETCH_STROKE5: fp32 rows (dx, dy, p_down, p_up, p_end), ld >= 5 T; a = argmax(row[2:5]), ties to the first index: the
 *       sketch ends before the first row with a == 2, the pen is lifted where a == 1 (metrics/samples.py: stroke5_to_stroke3).
 *     SKF_SKETCH_DICT_TOKENS: int64 ids, ld ids from sketch to sketch (>= T, the first T are read), centers (K, 2) fp32, contiguous;
 *       PAD = 0, SEP = K + 1, SOS = K + 2, EOS = K + 3 (utils/tokenizer.py: Tokenizer.decode_single): id 1 .. K appends the offset
 *       centers[id - 1], SEP lifts the pen on the previous point if there is one, EOS ends the sketch, SOS and PAD are skipped.
 *     SKF_SKETCH_GRID_TOKENS: int64 ids, K = the grid resolution R (even), n = R^2 ids with SEP = n + 1, SOS = n + 2, EOS = n + 3
 *       (GridTokenizer.decode_single): id 1 .. n is the ABSOLUTE position of its cell centre,
 *       (float)((double)((id - 1) % R) / (R / 2) - 1 + 1 / R) and the same of (id - 1) / R; SEP closes a line that has a point,
 *       EOS ends the sketch, and the last point's pen is lifted like the last line of the host decoder.
 *   Output: xy (B, T, 2) fp32 ABSOLUTE positions (for offsets the running sum from the origin, which is itself no point; summed as
 *   a shuffle scan per 64 positions plus a carry: exact whenever every partial sum is representable, otherwise within a few
 *   roundings per 64 positions), pen (B, T) bytes (1 = the pen lifts after this point), n_points (B), bounds (B, 4) fp32 =
 *   (min x, min y, max x, max y) over the points (zeros for an empty sketch).  Rows n_points[b] .. T - 1 of xy and pen are zeroed.
 *   Two deliberate differences from the host decoders: an empty sketch gives n_points = 0 (the host returns one dummy row), and
 *   a token id outside the vocabulary (negative, or above EOS) is skipped and never used as an index (the host raises).
 *   Limits (SKF_EINVAL): kind one of the four, B >= 1, 1 <= T < 2^31 / 5, ld as above, data aligned to its element, lengths for
 *   stroke-3, centers and K >= 1 for dictionary tokens, R even in [2, 32768] for grid tokens.  Offsets must be finite.
 * skf_rasterize_f32: points -> anti-aliased coverage images out (B, H, W) fp32, contiguous, ink = 1, paper = 0.  xy, pen, n_points
 *   as written above (n_points is clamped to [0, T]); frames (B, 4) = the box (x0, y0, x1, y1) each sketch is fitted into: with
 *   w = x1 - x0, h = y1 - y0 and the margin m in pixels, s = min((W - 2 m) / w, (H - 2 m) / h), a side below 1e-6 is left out of
 *   the min and s = 0 when both are; the pixel position of p is q = (W / 2, H / 2) + s (p - box centre), y grows downwards, row v
 *   of the image is pixel y = v.  Point i contributes the segment q[i-1] -> q[i] if i > 0 and pen[i-1] == 0, else the dot q[i].
 *   The coverage of pixel (u, v) is clamp(0.5 + line_width / 2 - d, 0, 1), d = the smallest Euclidean distance from its centre
 *   (u + 0.5, v + 0.5) to any primitive, all in fp32: points and pixel centres are both taken relative to (W / 2, H / 2) (the same
 *   distances from coordinates half as large), the foot point is t = clamp(((c - a) . (b - a)) / |b - a|^2, 0, 1) and
 *   c - a - t (b - a) is one fused multiply-add per coordinate.  n_points = 0 gives a blank image.  A primitive whose bounding box misses
 *   a 32 x 32 pixel tile grown by line_width / 2 + 0.5 is skipped for that tile (it cannot cover any of its pixels).
 *   Limits (SKF_EINVAL): H, W in [1, 16384], 0 < line_width <= 1024, margin >= 0, 2 margin < min(H, W), B, T >= 1.
 * skf_raster_overlap_f32: a, b (B, N) fp32 rows (N = H W) -> out (B, 2) = (sum min(a, b), sum max(a, b)) per pair, fp32, summed
 *   in a fixed order (a[i], b[i] with themselves give two identical sums).  Limits (SKF_EINVAL): B, N >= 1, lda, ldb >= N. */
#define SKF_SKETCH_STROKE3 0
#define SKF_SKETCH_STROKE5 1
#define SKF_SKETCH_DICT_TOKENS 2
#define SKF_SKETCH_GRID_TOKENS 3
int skf_sketch_points(int kind, const void* data, long long ld, const int* lengths, const float* centers, int K, int B, int T,
                      float* xy, unsigned char* pen, int* n_points, float* bounds, skf_stream_t stream);
int skf_rasterize_f32(const float* xy, const unsigned char* pen, const int* n_points, const float* frames, int B, int T, int H,
                      int W, float line_width, float margin, float* out, skf_stream_t stream);
int skf_raster_overlap_f32(const float* a, long long lda, const float* b, long long ldb, int B, long long N, float* out,
                           skf_stream_t stream);

/* ------------------------------------------------------------------ Sketch encoding (raw stroke-3 -> model input)
 * The direction a user meets first: raw stroke-3 sketches -> the (N, L) token rows / (N, L, 5) stroke-5 rows the model reads.  The
 * specification is the project's own host code - DistributedStroke3DataLoader.preprocess_per_sketch_from, Tokenizer.encode with a
 * .npz dictionary (float64 nearest_center, first minimum wins) and GridTokenizer.encode - and the results are BIT-EQUAL to it, not
 * close.  Two things decide that:
 *   - Summation order is part of the definition.  The bounds are a float64 running sum and the grid positions an fp32 running sum,
 *     one add per point in sequence; the fp32 sum is not order-free (a 64-wide shuffle scan plus carry put 88 of 800 coordinate
 *     rows of integer sketches into at least one other cell).  The scans are therefore sequential per sketch: one lane owns one
 *     sketch, the per-point work (nearest centre, scatter into the rows) runs point-parallel in launches of its own.
 *   - No contraction, no approximate division: every operation named below is rounded on its own (no fused multiply-add), and the
 *     divisions are correctly rounded fp32 divisions.
 * Nothing here allocates, synchronises with the host or uses an atomic; two calls on the same inputs agree bit for bit.
 * skf_nearest_center_f64: points (P, 2) fp32, ldp floats from row to row; centers (K, 2) fp64, contiguous; labels[i] (P int32) = the
 *   nearest centre of point i.  Per pair dx = (double)x - cx; dy = (double)y - cy; d = dx * dx + dy * dy, each of the operations
 *   rounded to fp64 on its own; among equal minima the lowest index wins.  (skf_kmeans_assign_f32 defines its distance as fp32 fmaf:
 *   the two can disagree, and the tokenizer's rule is this one.)  Limits (SKF_EINVAL): 1 <= K <= 4096, 1 <= P < 2^31, ldp >= 2.
 *   sklearn's own KMeans.predict may differ from this rule on exact near-ties.
 * skf_sketch_encode: flat (P, 3) fp32 rows (dx, dy, pen) of N sketches back to back, offsets (N + 1 int64, on the device,
 *   non-decreasing from 0 to P: sketch s owns rows offsets[s] .. offsets[s + 1] - 1; the caller checks that, the kernels only
 *   clamp what they read so that they stay in bounds).  flags & SKF_ENCODE_CLAMP: all three columns are clamped to +-1000 first
 *   (np.clip).  Per sketch, in this order and precision:
 *     bounds: running sums of (double)x and (double)y in sequence; min and max include the origin;
 *       div = (float)max(max_x - min_x, max_y - min_y, 1.0); X = x / div, Y = y / div in fp32.  scale (N fp32, NULL = not wanted)
 *       receives div.
 *     SKF_ENCODE_DICT: out (N, L) int64; id = nearest centre of (X, Y) by the rule above + 1; the row is SOS, every id followed by
 *       SEP where pen == 1, EOS; truncated to L, padded with PAD = 0; SEP = K + 1, SOS = K + 2, EOS = K + 3.
 *     SKF_ENCODE_GRID: out (N, L) int64; K is the resolution R (even); c = the sequential fp32 running sum of X (likewise Y),
 *       cell = (int)((c + 1.0f) * (float)(R / 2)) truncated toward zero, cell R -> R - 1, id = cell_x + cell_y * R + 1; SEP = R^2 + 1,
 *       SOS = R^2 + 2, EOS = R^2 + 3.  Points behind the last pen lift are dropped, unless the sketch has no lift: then all points
 *       and one SEP.  Truncation as for DICT.
 *     SKF_ENCODE_STROKE5: out (N, L, 5) fp32; rows (X, Y, 1 - pen, pen, 0) for the first min(n, L) points, (0, 0, 0, 0, 1) behind
 *       them, and column 4 of row L - 1 is always 1.
 *   An empty sketch gives an all-PAD row / all (0, 0, 0, 0, 1) rows and scale 1 (the host raises IndexError; the Python layers do
 *   so too, before the call).  Limits (SKF_EINVAL): N >= 1, 1 <= P < 2^31, L >= 2, 1 <= K <= 4096 (DICT), R even in [2, 32768]
 *   (GRID), unknown flag bits.  Inputs must be finite.  workspace: skf_sketch_encode_workspace_bytes(P, N) bytes (0 = bad sizes),
 *   16-byte aligned; its contents carry nothing from one call to the next. */
#define SKF_ENCODE_DICT 0
#define SKF_ENCODE_GRID 1
#define SKF_ENCODE_STROKE5 2
#define SKF_ENCODE_CLAMP 1u
int skf_nearest_center_f64(const float* points, int ldp, long long P, const double* centers, int K, int* labels,
                           skf_stream_t stream);
size_t skf_sketch_encode_workspace_bytes(long long P, int N);
int skf_sketch_encode(const float* flat, long long P, const long long* offsets, int N, int mode, const double* centers, int K,
                      int L, unsigned flags, void* out, float* scale, void* workspace, size_t workspace_bytes,
                      skf_stream_t stream);

/* ------------------------------------------------------------------ Sketch augmentation (random scale, point dropout)
 * The training augmentation of continuous sketches, in front of skf_sketch_encode.  The specification is the project's own host
 * code - DistributedStroke3DataLoader._augment_sketch (random_scale, then augment_strokes) - and the results are BIT-EQUAL to it.
 * There is no device random generator: the host draws, the device replays.  The reference draws np.random.random() twice per
 * sketch and once per point whether the draw is used or not, so the stream depends on the lengths alone and one host call
 * np.random.random(size = 2 N + P) yields it.  Nothing here allocates, synchronises with the host or uses an atomic; every output
 * element has one writer per launch; two calls on the same inputs agree bit for bit.
 * skf_sketch_augment: flat (P, 3) fp32 and offsets (N + 1 int64) as for skf_sketch_encode.  rnd: 2 N + P fp64 in the order the host
 *   draws them: sketch s owns rnd[offsets[s] + 2 s ..]: ux, uy, then one draw u per point.  out_flat has room for P rows (P, 3);
 *   out_offsets (N + 1 int64) receives the offsets of the augmented sketches, out_offsets[N] = the number of rows kept, P' <= P;
 *   rows P' .. P - 1 of out_flat are not written.  Per sketch, in this order and precision:
 *     flags & SKF_AUGMENT_CLAMP: all three columns are clamped to +-1000 first (np.clip);
 *     fx = (float)(((ux - 0.5) * 2.0) * scale_factor + 1.0), every operation in fp64, rounded to fp32 once; fy likewise from uy;
 *     x = x * fx, y = y * fy in fp32;
 *     the loop of augment_strokes over the points: prev = the pen of the last kept row, 1 before the first point; count = 0 where
 *       pen == 1 or prev == 1, else count + 1; a point is DROPPED when pen == 0 and prev == 0 and count > 2 and u < prob, u and
 *       prob compared in fp64.  The (x, y) of a dropped point are added to the last kept row in fp32, one add per point in point
 *       order (not the sum of the run added once); a kept point is copied, pen included.
 *   No fused multiply-add anywhere.  An empty sketch consumes its two draws and contributes no row.  Hand the result to
 *   skf_sketch_encode with P' as its P (its offsets must cover its flat exactly) and without SKF_ENCODE_CLAMP: the sketches were
 *   clamped before the augmentation, like the reference.
 *   Limits (SKF_EINVAL): N >= 1, 1 <= P < 2^31, 0 < prob <= 1, 0 <= scale_factor < 1, unknown flag bits, pointers not aligned to
 *   their element, a workspace below skf_sketch_augment_workspace_bytes(P, N) bytes (0 = bad sizes) or not 16-byte aligned; its
 *   contents carry nothing from one call to the next.  Inputs must be finite. */
#define SKF_AUGMENT_CLAMP 1u
size_t skf_sketch_augment_workspace_bytes(long long P, int N);
int skf_sketch_augment(const float* flat, long long P, const long long* offsets, int N, const double* rnd, double scale_factor,
                       double prob, unsigned flags, float* out_flat, long long* out_offsets, void* workspace,
                       size_t workspace_bytes, skf_stream_t stream);

/* ------------------------------------------------------------------ Stroke simplification (Ramer-Douglas-Peucker)
 * The step in front of everything above: raw drawings -> the simplified stroke-3 sketches the loaders read (QuickDraw's published
 * files are its raw drawings after RDP at epsilon 2.0; the reference pulls in the `rdp` package for user drawings).  The
 * specification is the project's own host restatement (tests/simplify_reference.py) and the results are BIT-EQUAL to it.
 * The rule.  A polyline of n points (x, y) in fp32, indices 0 .. n - 1.  Points 0 and n - 1 are kept; n <= 2 keeps everything.  A
 *   segment (a, b) with b - a >= 2 is examined so, the inputs widened to fp64 and every operation rounded to fp64 on its own (no
 *   fused multiply-add): ex = xb - xa, ey = yb - ya; for every interior i: px = xi - xa, py = yi - ya; if ex == 0 and ey == 0 (a
 *   closed or degenerate segment) m_i = px * px + py * py and L2 = 1, otherwise c = ex * py - ey * px, m_i = c * c and
 *   L2 = ex * ex + ey * ey; k = the LOWEST index with the largest m; if m_k > (epsilon * epsilon) * L2 (strict; epsilon * epsilon
 *   is one fp64 product) k is kept and (a, k) and (k, b) are examined, otherwise nothing between a and b is kept.  There is no
 *   division and no square root: for integer-valued coordinates (QuickDraw's 0 .. 255 grid) every quantity is an exact integer in
 *   fp64 and the result is exact RDP.  The kept set depends on the per-segment decisions alone, so the order in which segments are
 *   examined is free: the device examines all live segments of a recursion level at once, one wavefront per polyline, and needs
 *   as many levels as the recursion is deep (n - 1 for a zigzag of shrinking amplitude).
 * Nothing here allocates, synchronises with the host or uses an atomic; every output element has one writer per launch; two calls
 * on the same inputs agree bit for bit and a polyline's result does not depend on the rest of the batch.  Polyline length is not
 * limited: up to SKF_RDP_LDS_POINTS points a wavefront holds its polyline on chip, a longer one runs from the workspace with the
 * same result.  Inputs must be finite.
 * skf_rdp_f32: xy (P, 2) fp32 absolute points, ldp floats from row to row; stroke_offsets (S + 1 int64, on the device,
 *   non-decreasing from 0 to P: stroke s owns points stroke_offsets[s] .. stroke_offsets[s + 1] - 1; the caller checks that, the
 *   kernel clamps what it reads and never trusts it as an index).  keep (P bytes): 1 = kept, 0 = dropped, every byte a stroke owns
 *   is written exactly once; an empty stroke writes nothing.
 *   Limits (SKF_EINVAL): S >= 1, 1 <= P < 2^31, ldp >= 2, epsilon finite and >= 0, xy and stroke_offsets not aligned to their
 *   element, a workspace below skf_rdp_workspace_bytes(P) bytes (0 = bad size) or not 16-byte aligned; its contents carry
 *   nothing from one call to the next.
 * skf_stroke3_simplify: flat (P, 3) fp32 rows (dx, dy, pen) and offsets (N + 1 int64) as for skf_sketch_encode and
 *   skf_sketch_augment.  Per sketch, in this order:
 *     the absolute position A_j of row j is the sequential fp32 running sum of dx and of dy, one add per point (the grid
 *       tokenizer's rule); the position before the first row is (0, 0);
 *     a stroke is a run of rows that ends at a row with pen == 1, or at the sketch's last row;
 *     the rule above runs per stroke over its absolute points (stroke ends are always kept: pen values and the number of strokes
 *       do not change);
 *     a kept row j gives the output row (A_j - A_prev, pen_j), one fp32 subtraction per coordinate, A_prev the position of the
 *       kept row before it in the same sketch, (0, 0) for the first.
 *   out_flat has room for P rows (P, 3); out_offsets (N + 1 int64) receives the offsets of the simplified sketches,
 *   out_offsets[N] = the number of rows kept, P' <= P; rows P' .. P - 1 of out_flat are not written.  An empty sketch contributes
 *   no row.  flags: none defined, must be 0.
 *   Limits (SKF_EINVAL): N >= 1, 1 <= P < 2^31, epsilon finite and >= 0, flags != 0, pointers not aligned to their element, a
 *   workspace below skf_stroke3_simplify_workspace_bytes(P, N) bytes (0 = bad sizes) or not 16-byte aligned; its contents carry
 *   nothing from one call to the next. */
#define SKF_RDP_LDS_POINTS 512
size_t skf_rdp_workspace_bytes(long long P);
int skf_rdp_f32(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, double epsilon, unsigned char* keep,
                void* workspace, size_t workspace_bytes, skf_stream_t stream);
size_t skf_stroke3_simplify_workspace_bytes(long long P, int N);
int skf_stroke3_simplify(const float* flat, long long P, const long long* offsets, int N, double epsilon, unsigned flags,
                         float* out_flat, long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream);

/* ------------------------------------------------------------------ Arc-length resampling of polylines
 * The step Google's recipe for the simplified QuickDraw files runs in front of the simplification above (every stroke resampled
 * at a spacing of one pixel), and the classical cure for comparing drawings of different vertex density (a fixed number of points
 * equally spaced along the path, in front of skf_dtw_f32).  The reference has neither.  The specification is the project's own
 * host restatement (tests/resample_reference.py) and the results are BIT-EQUAL to it: every sum below is an integer sum and every
 * floating-point operation a single IEEE-rounded one, so a parallel evaluation and a sequential one agree.
 * The rule.  A polyline of n points p_0 .. p_{n-1}, absolute (x, y) in fp32.
 *   Segment lengths: dx = x_{i+1} - x_i, dy likewise, in fp32; c_i = sqrtf(dx * dx + dy * dy) in fp32, every operation rounded on
 *     its own (no fused multiply-add), the square root correctly rounded: the cost of skf_dtw_f32.
 *     q_i = (int64) rint((double) c_i * 2^16): lengths are integers in units of 2^-16 from here on.
 *   Arc-length table: C_0 = 0, C_{i+1} = C_i + q_i in int64; total = C_{n-1}.
 *   Spacing mode: s = rint(spacing * 2^16), s >= 1.  Targets T_m = m * s for every m >= 0 with T_m < total; the end point follows
 *     them.  The polyline gives ceil(total / s) + 1 rows: 1 row for total == 0 (a single point, or all points coincident).
 *   Count mode, n_out >= 2 rows: with total = a * (n_out - 1) + r, 0 <= r < n_out - 1: T_m = m * a + (m * r) / (n_out - 1) (integer
 *     division) for m = 0 .. n_out - 2: floor(m * total / (n_out - 1)) without a wide product.  The end point follows.  total == 0
 *     gives n_out copies of p_0.
 *   The sample at a target T: the segment is the i with C_i <= T < C_{i+1} (unique; a segment with q_i == 0 is never chosen);
 *     u = (double)(T - C_i) / (double) q_i; x = (float)((double) x_i + u * ((double) x_{i+1} - (double) x_i)), y likewise: the
 *     division, the multiply and the add are each rounded to fp64 on their own, then once to fp32.
 *   The end point is p_{n-1} copied bit for bit; the first row is p_0 bit for bit whenever there are two rows or more (u = 0).
 * Coordinates.  total cannot overflow int64 while every |x|, |y| <= SKF_RESAMPLE_MAX_COORD = 2^14: then c_i < 2^16, q_i < 2^32, and
 *   fewer than 2^31 of them add up to less than 2^63.  Stated, not checked here (ops.polyline_resample and simplify.resample_lines
 *   refuse larger coordinates on the host); inputs must be finite.  Whatever the inputs hold, no kernel leaves its buffers.
 * Nothing here allocates, synchronises with the host or uses an atomic; every output element has one writer per launch; two calls
 * on the same inputs agree bit for bit and a polyline's result does not depend on the rest of the batch.  Polyline length is not
 * limited.  xy (P, 2) fp32, ldp floats from row to row; stroke_offsets (S + 1 int64, on the device) as for skf_rdp_f32: the caller
 * checks them, the kernels clamp every range to [0, P] and never trust an offset as an index.
 * skf_polyline_resample_count: the measure launch (one wavefront per polyline: q_i, a wave scan with a carry from one tile of 64
 *   points to the next, C for every point into the workspace, the polyline's row count) and the counts -> offsets scan.  Afterwards
 *   out_offsets (S + 1 int64) holds the offsets of the resampled polylines, out_offsets[S] = the number of output rows P', and
 *   the workspace holds C.  An empty polyline gives no row.  A polyline's count saturates at 2^31 - 1: P' >= 2^31 - 1 means that
 *   the result does not fit and must not be emitted.
 * skf_polyline_resample_emit: the emit launch.  Same xy, ldp, P, stroke_offsets, S, spacing and the workspace exactly as _count
 *   left it; out_offsets as _count wrote them.  Row out_offsets[s] + m of out_xy (out_rows, 2) receives sample m of polyline s: one
 *   lane per row, consecutive lanes consecutive targets, the segment found by binary search over the polyline's slice of C.
 *   out_rows is the capacity: rows at or past it are not written, nor is any row a polyline does not own.
 * skf_polyline_resample_n: count mode in one call, out_xy (S, n_out, 2) dense.  An EMPTY polyline gives n_out rows (0, 0): the
 *   single point (0, 0) that stands for an empty sketch in skf_dtw_f32 and skf_shape_distance_f32.
 * Limits (SKF_EINVAL): S >= 1, 1 <= P < 2^31, ldp >= 2, spacing finite, below 7e13 and rint(spacing * 2^16) >= 1,
 *   2 <= n_out <= SKF_RESAMPLE_MAX_N, 1 <= out_rows < 2^31 (so P' < 2^31), xy not 4-byte, the offsets and out_xy not 8-byte
 *   aligned, a workspace below skf_polyline_resample_workspace_bytes(P, S) bytes (0 = bad sizes) or not 16-byte aligned. */
#define SKF_RESAMPLE_MAX_N 65536
#define SKF_RESAMPLE_MAX_COORD 16384
size_t skf_polyline_resample_workspace_bytes(long long P, int S);
int skf_polyline_resample_count(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, double spacing,
                                long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream);
int skf_polyline_resample_emit(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, double spacing,
                               const long long* out_offsets, float* out_xy, long long out_rows, void* workspace,
                               size_t workspace_bytes, skf_stream_t stream);
int skf_polyline_resample_n(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, int n_out, float* out_xy,
                            void* workspace, size_t workspace_bytes, skf_stream_t stream);

/* ------------------------------------------------------------------ Path flattening (lines and cubic Bezier segments -> polylines)
 * The door for vector drawings that are not polylines: SVG paths (sketchformer_amd/svg.py parses them on the host into lines and
 * cubics; quadratics and arcs arrive as cubics) become polylines under a stated error bound, and go straight into skf_rdp_f32 and
 * skf_polyline_resample_*.  The reference samples a path by its length through svgpathtools (utils/skt_tools.py: read_svg); the
 * specification here is the project's own host restatement (tests/flatten_reference.py) and the results are BIT-EQUAL to it.
 * Inputs.  ctrl (G, 4, 2) fp64: the control points p0 .. p3 of G segments, absolute (x, y).  kind (G int32): 1 = cubic; 0 = line,
 *   of which only p0 and p3 count; ANY OTHER VALUE IS TREATED AS 0.  path_offsets (S + 1 int64, on the device): subpath s owns the
 *   segments [path_offsets[s], path_offsets[s + 1]); the caller checks them, the kernels clamp every range to [0, G] and never
 *   trust an offset as an index.  tol > 0, in the units of ctrl; the host forms c = (16 / 9) * tol^2 once in fp64 (16.0 / 9.0,
 *   tol * tol, then their product: three roundings).
 * Pieces per segment, n.  A line has n = 1.  A cubic: ax = (x0 - 2 x1) + x2, bx = (x1 - 2 x2) + x3, ay and by likewise;
 *   dd = max(ax * ax + ay * ay, bx * bx + by * by), every fp64 operation rounded on its own, a NaN on either side giving a NaN.
 *   n is the smallest integer in [1, SKF_FLATTEN_MAX_N] with (double)(n * n) * (double)(n * n) * c >= dd, and SKF_FLATTEN_MAX_N if
 *   there is none (so for a NaN or an infinite dd).  n^4 is exact in fp64 up to 2^13 and the test is monotone in n: how n is
 *   searched for does not change it.  It is the bound of uniform subdivision, 0.75 * M / n^2 <= tol with M = max(|a|, |b|), the
 *   second differences of the control polygon, without a square root or a division.
 * Rows.  A subpath with at least one segment gives 1 + sum(n) rows: first (float) p0 of its first segment; then segment k gives n
 *   rows, j = 1 .. n.  For j < n: t = (double) j / (double) n and de Casteljau with lerp(a, b) = a + t * (b - a), six lerps a
 *   coordinate in the order q0 = lerp(p0, p1), q1 = lerp(p1, p2), q2 = lerp(p2, p3), r0 = lerp(q0, q1), r1 = lerp(q1, q2),
 *   s = lerp(r0, r1): every operation rounded to fp64 on its own (no fused multiply-add), then s is cast once to fp32.  Row n is
 *   (float) p3, copied and not evaluated: a join repeats no row and skips none, whether or not p3 of one segment equals p0 of the
 *   next (only the first segment's p0 is ever read as a row).  An empty subpath gives no row.
 * Nothing here allocates, synchronises with the host or uses an atomic; every output element has one writer per launch; two calls
 * on the same inputs agree bit for bit and a subpath's rows do not depend on the rest of the batch.  Subpath length is not limited.
 * skf_path_flatten_count: the count launch (one wavefront per subpath: n per segment, a wave scan with a carry from one tile of 64
 *   segments to the next, the inclusive running sum of n for every segment into the workspace, the subpath's row count) and the
 *   counts -> offsets scan.  Afterwards out_offsets (S + 1 int64) holds the offsets of the flattened subpaths, out_offsets[S] = the
 *   number of output rows P'.  A subpath's count saturates at 2^31 - 1: P' >= 2^31 - 1 means that the result does not fit and must
 *   not be emitted.
 * skf_path_flatten_emit: the emit launch.  Same ctrl, kind, G, path_offsets, S, tol and the workspace exactly as _count left it;
 *   out_offsets as _count wrote them.  Row out_offsets[s] + m of out_xy (out_rows, 2) receives row m of subpath s: one lane per
 *   row, consecutive lanes consecutive rows, the segment found by binary search over the subpath's slice of the running sums.
 *   out_rows is the capacity: rows at or past it are not written, nor is any row a subpath does not own.
 * Limits (SKF_EINVAL): a null pointer, S >= 1, 1 <= G < 2^31, tol finite and > 0, 1 <= out_rows < 2^31 (so P' < 2^31), ctrl,
 *   path_offsets, out_offsets and out_xy not 8-byte, kind not 4-byte aligned, a workspace below
 *   skf_path_flatten_workspace_bytes(G, S) bytes (0 = bad sizes) or not 16-byte aligned. */
#define SKF_FLATTEN_MAX_N 4096
size_t skf_path_flatten_workspace_bytes(long long G, int S);
int skf_path_flatten_count(const double* ctrl, const int* kind, long long G, const long long* path_offsets, int S, double tol,
                           long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream);
int skf_path_flatten_emit(const double* ctrl, const int* kind, long long G, const long long* path_offsets, int S, double tol,
                          const long long* out_offsets, float* out_xy, long long out_rows, void* workspace, size_t workspace_bytes,
                          skf_stream_t stream);

/* ------------------------------------------------------------------ Stroke edits (permute, reverse, drop)
 * New sketches built out of the strokes of old ones: the strokes in any order, forwards or backwards, some left out or repeated,
 * the pen jumps between them recomputed.  It is what the reference loader's shuffle_stroke option does on the host through
 * polylines and back, and what a study of stroke order, stroke direction and stroke importance multiplies a batch with.  The
 * specification is the project's own host restatement (tests/strokes_reference.py) and the results are BIT-EQUAL to it.
 * The rule.  flat (P, 3) fp32 rows (dx, dy, pen) and offsets (N + 1 int64) as for skf_sketch_encode.
 *   Strokes: within a sketch a stroke is a maximal run of rows that ends at a row with pen == 1, or at the sketch's last row
 *     (skf_stroke3_simplify's definition).  An empty sketch has no strokes; a stroke is never empty.
 *   Absolute positions: A_j is the sequential fp32 running sum of dx and of dy, one add per point, from (0, 0)
 *     (skf_stroke3_simplify's rule).
 *   The stroke table: sketch_strokes (N + 1 int64): sketch s owns the global strokes sketch_strokes[s] .. sketch_strokes[s + 1] - 1,
 *     T = sketch_strokes[N] <= P; stroke_rows (T + 1 int64): the first flat row of every stroke, stroke_rows[T] = the number of
 *     rows; stroke_ends (T, 4) fp32: A of the stroke's first row and of its last row, (x, y, x, y).
 *   An edit describes M output sketches: src (M int32) names the source sketch of each, sel_offsets (M + 1 int64) delimits its
 *     selection list in sel (Q int32).  An entry k >= 0 selects stroke k of the source sketch, drawn as stored; ~k (= -k - 1)
 *     selects the same stroke drawn backwards.  Strokes may repeat, a list may be empty, M may be smaller or larger than N.  An
 *     entry that names no stroke - src outside [0, N), or k at or past the source's stroke count - is ABSENT: it gives no rows,
 *     and the entries around it join as if it had not been listed.
 *   Output rows: a selected stroke with the source rows a .. b gives b - a + 1 rows.  E = the position where the previous
 *     present entry of the same list ended, (0, 0) for the first.
 *     Forward: the first row is A_a - E, one fp32 subtraction per coordinate; the rows a + 1 .. b follow with dx, dy copied bit for
 *       bit; the stroke ends at A_b.
 *     Backward: the first row is A_b - E; then for i = b down to a + 1 a row (-dx_i, -dy_i): a sign flip of the stored bits, so a
 *       stored +0 becomes -0; the stroke ends at A_a.
 *     Pen: 1 on the stroke's last output row, 0 on the others: the identity edit differs from its input only in the pen of an
 *       unterminated final stroke (and in pen values other than 0 and 1, which end no stroke).
 *     No fused multiply-add anywhere (there is no product to fuse; the file is compiled like its neighbours all the same).
 *   Consequences.  E and the stroke ends come from the source's A, not from re-summing output rows, so a stroke's rows depend on
 *     nothing but its own sketch and the entry in front of it.  Inside a stroke nothing is rounded.  On integer-valued data below
 *     2^24 (raw QuickDraw) every sum is exact and the identity edit returns its input bit for bit.  On other data a jump - the
 *     first row of a stroke - can differ from the stored offset by one fp32 rounding (A_a - A_{a-1} need not give back dx_a), and
 *     a stored -0 in a stroke's first row comes back as +0.
 * Nothing here allocates, synchronises with the host or uses an atomic; every output element has one writer per launch; two calls
 * on the same inputs agree bit for bit.  Every range read from offsets, sketch_strokes, stroke_rows, src, sel_offsets or sel is
 * clamped before it is used as an index: no input can take a kernel out of its buffers.  The caller checks that offsets and
 * sel_offsets are non-decreasing from 0 to P and to Q (lists that overlap would give an entry two writers).
 * skf_stroke_table: one wavefront per sketch counts its strokes with ballots over tiles of 64 rows, the counts -> offsets scan
 *   writes sketch_strokes, and a second launch writes stroke_rows and stroke_ends: a stroke's rank within the sketch is a popcount
 *   below the lane plus the tile carry, the positions come from one lane's sequential walk.  stroke_rows has room for P + 1
 *   entries and stroke_ends for P rows; the entries 0 .. T of stroke_rows and the rows 0 .. T - 1 of stroke_ends are written.
 *   flags: none defined, must be 0.
 * skf_stroke_edit_count: the table's sketch_strokes (N + 1), stroke_rows (T + 1) and T as the caller read it back; src,
 *   sel_offsets, sel as above.  One wavefront per output sketch gives every entry its stroke (or none), its length and, through a
 *   wave scan over the list in tiles of 64 entries with a carry, its first output row; the counts -> offsets scan follows.
 *   Afterwards out_offsets (M + 1 int64) holds the offsets of the output sketches, out_offsets[M] = the number of output rows
 *   P', and the workspace holds what _emit reads.  A sketch's count saturates at 2^31 - 1: P' >= 2^31 - 1 means that the result does
 *   not fit and must not be emitted.
 * skf_stroke_edit_emit: the same arguments and the workspace exactly as _count left it, plus flat and stroke_ends (T, 4);
 *   out_offsets as _count wrote them.  A wavefront takes 64 entries at a time: every lane gathers one entry's header, then every
 *   lane writes one row of out_flat (out_rows, 3) at a time, consecutive lanes consecutive rows, the owning entry found by binary
 *   search over the 64 starts on chip.  out_rows is the capacity: rows at or past it are not written, nor is any row no stroke
 *   owns.
 * Limits (SKF_EINVAL): N, M >= 1, 1 <= P < 2^31, 0 <= Q < 2^31, 0 <= T <= P, 1 <= out_rows < 2^31, flags != 0, a pointer not
 *   aligned to its element, a workspace below skf_stroke_table_workspace_bytes(P, N) / skf_stroke_edit_workspace_bytes(P, N, M, Q)
 *   bytes (0 = bad sizes) or not 16-byte aligned; its contents carry nothing from one call to the next, other than from _count to
 *   _emit.  sel may be null when Q == 0, stroke_ends when T == 0. */
size_t skf_stroke_table_workspace_bytes(long long P, int N);
int skf_stroke_table(const float* flat, long long P, const long long* offsets, int N, unsigned flags, long long* sketch_strokes,
                     long long* stroke_rows, float* stroke_ends, void* workspace, size_t workspace_bytes, skf_stream_t stream);
size_t skf_stroke_edit_workspace_bytes(long long P, int N, int M, long long Q);
int skf_stroke_edit_count(long long P, const long long* sketch_strokes, int N, const long long* stroke_rows, long long T,
                          const int* src, const long long* sel_offsets, int M, const int* sel, long long Q, unsigned flags,
                          long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream);
int skf_stroke_edit_emit(const float* flat, long long P, const long long* sketch_strokes, int N, const long long* stroke_rows,
                         const float* stroke_ends, long long T, const int* src, const long long* sel_offsets, int M, const int* sel,
                         long long Q, unsigned flags, const long long* out_offsets, float* out_flat, long long out_rows,
                         void* workspace, size_t workspace_bytes, skf_stream_t stream);

/* ------------------------------------------------------------------ Sequence alignment (token edit distance, point DTW)
 * The reference has nothing in this place: it judges a reconstruction by eye (metrics/samples.py) and its README's retrieval has
 * no classical baseline.  What is compared here is what the model emits: the ids that models/sketchformer.py `predict` returns
 * against the ids of utils/tokenizer.py, and the pen positions both decode to (skf_sketch_points).  Both distances are O(La Lb)
 * dynamic programs per pair; one wavefront sweeps a pair's table as a systolic array (a strip of columns per lane, one cross-lane
 * move per row), with no table in memory.  Nothing here allocates, synchronises with the host or uses an atomic; two calls on the
 * same inputs agree bit for bit and a pair's result does not depend on the rest of the batch.
 * Shared rules.  cross == 0: Na == Nb, out is (Na) and pairs row i of a with row i of b.  cross == 1: out is (Na, Nb) row-major
 *   and holds every (i, j).  len_* / n_* are int32 on the device, one per row; they are clamped to [0, T] inside the kernel and never
 *   trusted as an index.  Elements behind a row's length are never read into a result.  lda, ldb: elements of the row's type
 *   (ids; floats) from row to row.  Limits (SKF_EINVAL): Na, Nb >= 1; 1 <= Ta, Tb <= SKF_ALIGN_MAX_LEN; lda >= Ta, ldb >= Tb (ids),
 *   lda >= 2 Ta, ldb >= 2 Tb (points); a, b 8-byte aligned (ids), xy_a, xy_b, the lengths and out 4-byte aligned; cross in {0, 1};
 *   cross == 0 with Na != Nb; cross == 1 with Na * ceil(Nb / 4) >= 2^31.
 * skf_edit_distance_i64: unit-cost Levenshtein distance (insert, delete, substitute = 1) between ids a[i, 0 .. len_a[i]) and
 *   b[j, 0 .. len_b[j]): D(0, j) = j, D(i, 0) = i, D(i, j) = min(D(i-1, j) + 1, D(i, j-1) + 1, D(i-1, j-1) + (a_i != b_j)), the
 *   result is D(len_a, len_b).  Ids are compared as full 64-bit integers.  An empty side gives the other side's length.  Results
 *   are int32 and exact.
 * skf_dtw_f32: dynamic time warping between the point rows xy_a[i] and xy_b[j]: (x, y) fp32 pairs as skf_sketch_points writes them
 *   (the pen byte plays no part), n_a[i] and n_b[j] of them.  Local cost c(i, j) = sqrt(dx * dx + dy * dy), dx = ax - bx,
 *   dy = ay - by: every operation rounded to fp32 on its own, no fused multiply-add, the square root correctly rounded.
 *   D(0, 0) = c(0, 0); D(i, 0) = c(i, 0) + D(i-1, 0); D(0, j) = c(0, j) + D(0, j-1);
 *   D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)); the result is D(n_a - 1, n_b - 1), not normalised.  An empty side is
 *   replaced by the single point (0, 0), the dummy row the host decoders return for an empty sketch.  Every cell is one fixed
 *   fp32 expression of its three neighbours (min is exact), so the result does not depend on the order of the sweep: a float32
 *   numpy restatement matches it BIT FOR BIT.  Non-finite inputs are the caller's error (a NaN or an infinity in a row makes the
 *   results of its pairs meaningless; nothing else is affected). */
#define SKF_ALIGN_MAX_LEN 512
int skf_edit_distance_i64(const long long* a, long long lda, const int* len_a, int Na, int Ta, const long long* b, long long ldb,
                          const int* len_b, int Nb, int Tb, int cross, int* out, skf_stream_t stream);
int skf_dtw_f32(const float* xy_a, long long lda, const int* n_a, int Na, int Ta, const float* xy_b, long long ldb, const int* n_b,
                int Nb, int Tb, int cross, float* out, skf_stream_t stream);

/* ------------------------------------------------------------------ Teacher-forced scoring (sequence log-likelihood, rank)
 * The reference has nothing in this place: its surface stops at predict.  The decoders above produce sequences; this entry answers
 * the opposite question - how likely is a GIVEN sequence under the logits skf_model_forward left in the 'logits' buffer - with one
 * read of every logit that counts and none of the others.  skf_softmax_ce is the training kernel (in-place gradient, PAD mask, no
 * rank, no per-sequence sum); this one only reads.  Nothing here allocates, synchronises with the host or uses an atomic; two
 * calls on the same inputs agree bit for bit and a sequence's results depend neither on B, nor on its slot, nor on its neighbours.
 * skf_sequence_score: row b * T + t of logits (pitch ld elements; float32, or bf16 with is_bf16 = 1, widened exactly) is the
 *   distribution over the token at target position y = target[b * tgt_ld + tgt_off + t].
 *   Scored length n_b (the `length` of skf_model_beam_decode): with t* the first position whose y == eos, n_b = t* + 1 (the EOS
 *     itself is scored); without one, n_b = the first position whose y == 0 (PAD); without either, n_b = T.  seq_len[b] = n_b.
 *   Scored positions, t < n_b:  tok_logp[b, t] = z_y - m - log sum_j exp(z_j - m), m the row maximum, in float32;
 *     tok_rank[b, t] = #{j : z_j > z_y} + #{j < y : z_j == z_y}: rank 0 is the first-index-argmax hit of
 *     builders/keras_metrics.py:25 that skf_softmax_ce reports as row_hit.
 *   Unscored positions, t >= n_b:  tok_logp = 0.0f, tok_rank = -1; their logits rows and their targets are NOT READ (they may hold
 *     anything, NaN included).
 *   seq_logp[b] = the float32 sum of the stored tok_logp[b, 0 .. n_b - 1], added one at a time in ascending t from 0.0f (n_b = 0
 *     gives 0.0f): a float32 host loop over tok_logp gives the same bits.
 *   Edge rules.  A target outside [0, V) is never used as an index: the position scores -inf with rank V (its row is not read).
 *     -inf logits are legal: under a finite row maximum a -inf target scores -inf (not NaN) and other -inf entries add 0 to the sum.
 *     A row that is all -inf, or holds +inf or a NaN, is outside the contract (the position's results are meaningless; nothing
 *     else is affected).  The maximum is subtracted before every exp: rows around +80 or -80 score like rows around 0.
 *   Rows whose base and pitch are 16-byte aligned (ld % 4 == 0 in float32, ld % 8 == 0 in bf16) are read 16 bytes per lane, any
 *     other pitch element by element; the results do not depend on which.
 *   Limits (SKF_EINVAL): B, T, V >= 1; B * T < 2^31; ld >= V; tgt_off >= 0 and tgt_ld >= tgt_off + T; is_bf16 in {0, 1}; logits
 *     aligned to its element, target 8-byte and the four outputs (tok_logp, tok_rank (B, T); seq_logp, seq_len (B)) 4-byte aligned. */
int skf_sequence_score(const void* logits, int is_bf16, int ld, int B, int T, int V, const long long* target, int tgt_ld, int tgt_off,
                       long long eos, float* tok_logp, int* tok_rank, float* seq_logp, int* seq_len, skf_stream_t stream);

/* ------------------------------------------------------------------ Order-free shape distances (Chamfer, Hausdorff)
 * The reference has nothing in this place.  The alignment distances above compare sequences - the same ink in another stroke order
 * is far away - and the raster overlap is tied to a resolution and a line width.  This entry measures how far the INK of one sketch
 * lies from the ink of another: per pair the mean and the maximum, both ways, of the distance from the samples of one sketch to the
 * nearest primitive of the other; the Chamfer and the Hausdorff distance follow from the four numbers.  One workgroup keeps sketch a
 * resident in LDS against a block of rows of b and computes both directions where both are resident; the (samples x primitives)
 * table never exists.  Nothing here allocates, synchronises with the host or uses a floating-point atomic; two calls on the same
 * inputs agree bit for bit and a pair's result does not depend on the rest of the batch.
 * skf_shape_distance_f32.  A sketch is what skf_sketch_points writes: xy (T, 2) fp32 absolute positions, pen (T) bytes (1 = the pen
 *   lifts after this point) and n points, clamped to [0, T] inside the kernel and never trusted as an index; what lies behind n is
 *   never read.  An empty sketch (n = 0) stands for the single point (0, 0) with its pen lifted, as for skf_dtw_f32.
 *   Primitives of a sketch: every point i < n is a dot p[i]; every i > 0 with pen[i-1] == 0 is in addition the segment a = p[i-1] to
 *     b = p[i], with e = b - a, len2 = ex * ex + ey * ey, inv = len2 > 0 ? 1.0f / len2 : 0.0f (a correctly rounded division).
 *   Samples of a sketch, for samples_per_segment = S in [1, 16]: every point p[i], used exactly; every segment adds the S - 1
 *     interior samples a + t * e, t = (float)j / (float)S, j = 1 .. S - 1.  count = n + (S - 1) * segments, or 1 for an empty sketch.
 *   Distance of a sample s to a sketch: d2 = the minimum over the sketch's primitives of
 *     dot:      qx * qx + qy * qy, q = s - p;
 *     segment:  px = sx - ax, py = sy - ay; dot = px * ex + py * ey; t = min(max(dot * inv, 0), 1); rx = px - t * ex, ry = py - t * ey;
 *               rx * rx + ry * ry;
 *     then d = sqrt(d2), correctly rounded.  Every operation is rounded to fp32 on its own, no fused multiply-add; the minimum is
 *     exact, so the order of the primitives plays no part.
 *   Directed results a -> b: max_ab = the largest d over the samples of a (exact);
 *     mean_ab = (float)(((double)Q / 16777216.0) / (double)count_a), Q = the int64 sum over the samples of a of
 *     (long long)floor((double)d * 16777216.0): an exact, order-free fixed-point sum (the device of skf_sample.h's masses).
 *   out holds four fp32 per pair: (mean_ab, mean_ba, max_ab, max_ba).  Chamfer = 0.5f * (mean_ab + mean_ba) and
 *     Hausdorff = max(max_ab, max_ba) are taken by the caller.  A float32 numpy restatement matches all four BIT FOR BIT.
 *   Contract (stated, not checked): the coordinates are finite, |c| <= 2^20, and no segment is so short that len2 underflows to a
 *     subnormal whose reciprocal is infinite.  A NaN spoils the results of its own pairs only.
 *   cross == 0: Na == Nb, out is (Na, 4) and pairs row i of a with row i of b.  cross == 1: out is (Na, Nb, 4) row-major.
 *   lda, ldb: floats from row to row of xy; ldpa, ldpb: bytes from row to row of pen.
 *   Limits (SKF_EINVAL): Na, Nb >= 1; 1 <= Ta, Tb <= SKF_ALIGN_MAX_LEN; lda >= 2 Ta, ldb >= 2 Tb, ldpa >= Ta, ldpb >= Tb; xy_a, xy_b,
 *     n_a, n_b 4-byte and out 16-byte aligned; S in [1, 16]; cross in {0, 1}; cross == 0 with Na != Nb; cross == 1 with
 *     Na * Nb * 4 >= 2^31. */
int skf_shape_distance_f32(const float* xy_a, long long lda, const unsigned char* pen_a, long long ldpa, const int* n_a, int Na, int Ta,
                           const float* xy_b, long long ldb, const unsigned char* pen_b, long long ldpb, const int* n_b, int Nb, int Tb,
                           int samples_per_segment, int cross, float* out, skf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SKF_H_ */
