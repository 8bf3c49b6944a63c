// Teacher-forced scoring (include/skf.h: skf_sequence_score): the log-likelihood and the rank of every target token under the
// logits the forward left behind, and their sum per sequence.  The reference has nothing in this place (its surface stops at
// predict); the specification is the float64 restatement of tests/score_reference.py.  DESIGN.md section 3q.
//
// Three launches on the caller's stream, no workspace, no atomic, no host synchronisation:
//   1. score_len_kernel   one wave per sample scans its targets once and writes n_b (seq_len);
//   2. score_rows_kernel  one wave (V <= SCORE_WIDE_V) or one workgroup of four waves per logits row.  A row at t >= n_b stores
//                         0.0f / -1 and is not read.  A scored row fetches z_y (one element, the same address in every lane) and then
//                         reads every logit exactly once, 16 bytes per lane where the row base and the pitch allow: each lane keeps
//                         a running maximum m, the sum s of exp(z - m) rescaled whenever m grows, and the count of the entries
//                         that rank in front of the target; the lanes are combined with wave64 shuffles (the four waves of a wide
//                         row through 12 words of LDS, in a fixed order);
//   3. score_sum_kernel   one wave per sample adds the STORED tok_logp of its n_b positions one at a time in ascending t (the
//                         values travel through v_readlane, the adds are a serial chain by construction), so seq_logp is bit-equal
//                         to a float32 host loop over tok_logp and depends on nothing but the sequence's own rows.
// Every reduction has a fixed order: two calls on the same inputs agree bit for bit, and a row's result does not depend on B, on
// its slot or on its neighbours.  Registers and LDS as compiled: profiles/score_build.txt.
#include "skf_common.h"
#include "skf_bf16.h"

namespace {

constexpr int SCORE_WAVES = 4;
constexpr int SCORE_THREADS = SCORE_WAVES * SKF_WAVE;
constexpr int SCORE_WIDE_V = 4096;      // above: a whole workgroup per row

__device__ __forceinline__ int wave_count(int v) {      // (an int overload of wave_sum here would hide skf_common.h's)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- 1. the scored length
// n_b = (first t with y == eos) + 1, else the first t with y == 0, else T.  One wave per sample, 64 targets per step.
__global__ __launch_bounds__(SCORE_THREADS) void score_len_kernel(const long long* __restrict__ target, int tgt_ld, int tgt_off, long long eos,
                                                                  int B, int T, int* __restrict__ seq_len) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const long long* row = target + (size_t)b * tgt_ld + tgt_off;
  int first_pad = T, n = -1;
  for (int base = 0; base < T; base += SKF_WAVE) {
    const int t = base + lane;
    const long long y = t < T ? row[t] : 1ll;            // behind the row: neither PAD ...
    const unsigned long long is_eos = __ballot(t < T && y == eos);      // ... nor EOS, whatever eos is
    const unsigned long long is_pad = __ballot(y == 0);
    if (first_pad == T && is_pad) first_pad = base + __builtin_ctzll(is_pad);
    if (is_eos) {
      n = base + __builtin_ctzll(is_eos) + 1;
      break;
    }
  }
  if (lane == 0) seq_len[b] = n >= 0 ? n : first_pad;
}

// ---------------------------------------------------------------- 2. one row
// What a lane has seen of its row: the maximum m, s = sum of exp(z - m) (m == -inf: nothing finite yet, s == 0), and how many
// entries rank in front of the target: z > z_y, or z == z_y at a lower index - which is z >= z_y in front of column y and z > z_y
// behind it, one compare per entry; only the one chunk that holds column y itself looks at indices.
// exp(z - m) is exp2(z * log2(e) - m * log2(e)), one fused multiply-add and one v_exp_f32 per entry; the product m * log2(e) is
// rounded once per chunk, an error of at most |m| * 2^-24 in the exponent that every term of the row shares: below 3 % of the
// bound the tests hold tok_logp to, whatever the magnitude of the row.
constexpr float SCORE_LOG2E = 1.44269504088896340736f;
__device__ __forceinline__ float score_exp(float x) { return __builtin_amdgcn_exp2f(x * SCORE_LOG2E); }     // exp2(-inf) = 0
struct RowAcc {
  float m, s;
  int ahead;
  template <int N>
  __device__ __forceinline__ void add(const float (&z)[N], int j0, float zy, int y) {
    float cm = z[0];
#pragma unroll
    for (int k = 1; k < N; ++k) cm = fmaxf(cm, z[k]);
    if (cm > m) {                                       // cm is finite (or the row is outside the contract)
      s *= score_exp(m - cm);                           // m == -inf: exp gives 0 and s was 0
      m = cm;
    }
    const float ml = (m == -__builtin_inff() ? 0.0f : m) * SCORE_LOG2E;      // only -inf so far: exp2(-inf - 0) = 0, never -inf - -inf
#pragma unroll
    for (int k = 0; k < N; ++k) s += __builtin_amdgcn_exp2f(__builtin_fmaf(z[k], SCORE_LOG2E, -ml));
    const int d = y - j0;                               // where column y lies, seen from this chunk
    if (d >= N) {
#pragma unroll
      for (int k = 0; k < N; ++k) ahead += z[k] >= zy ? 1 : 0;
    } else if (d < 0) {
#pragma unroll
      for (int k = 0; k < N; ++k) ahead += z[k] > zy ? 1 : 0;
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) ahead += (z[k] > zy || (z[k] == zy && k < d)) ? 1 : 0;
    }
  }
};

template <bool BF16> struct ScoreElem;
template <> struct ScoreElem<false> {
  typedef float T;
  static constexpr int VEC = 4;                         // elements per 16-byte load
  static __device__ __forceinline__ float widen(float v) { return v; }
  static __device__ __forceinline__ void load(const float* p, float (&z)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
  }
};
template <> struct ScoreElem<true> {
  typedef unsigned short T;
  static constexpr int VEC = 8;
  static __device__ __forceinline__ float widen(unsigned short v) { return skf_bf2f(v); }   // exact
  static __device__ __forceinline__ void load(const unsigned short* p, float (&z)[8]) { skf_unpack8(*reinterpret_cast<const uint4*>(p), z); }
};

// ROW_WAVES waves share a row; a workgroup holds SCORE_WAVES / ROW_WAVES rows.  vec: 16-byte loads are legal (the launcher checked
// the base and the pitch).
template <bool BF16, int ROW_WAVES>
__global__ __launch_bounds__(SCORE_THREADS) void score_rows_kernel(const typename ScoreElem<BF16>::T* __restrict__ logits, int ld, int rows,
                                                                   int T, int V, int vec, const long long* __restrict__ target, int tgt_ld,
                                                                   int tgt_off, const int* __restrict__ seq_len,
                                                                   float* __restrict__ tok_logp, int* __restrict__ tok_rank) {
  typedef ScoreElem<BF16> E;
  constexpr int ROWS = SCORE_WAVES / ROW_WAVES, VEC = E::VEC;
  __shared__ float sM[SCORE_WAVES], sS[SCORE_WAVES];
  __shared__ int sA[SCORE_WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int part = wave % ROW_WAVES;                    // this wave's share of the row
  const int r = blockIdx.x * ROWS + wave / ROW_WAVES;   // (with ROW_WAVES == 4 the same in all four waves: they leave together)
  if (r >= rows) return;
  const int b = r / T, t = r - b * T;
  const bool writer = lane == 0 && part == 0;
  if (t >= seq_len[b]) {                                // behind the sequence: the row is not read
    if (writer) {
      tok_logp[r] = 0.0f;
      tok_rank[r] = -1;
    }
    return;
  }
  const long long y64 = target[(size_t)b * tgt_ld + tgt_off + t];
  if (y64 < 0 || y64 >= V) {                            // never an index
    if (writer) {
      tok_logp[r] = -__builtin_inff();
      tok_rank[r] = V;
    }
    return;
  }
  const int y = (int)y64;
  const typename E::T* row = logits + (size_t)r * ld;
  const float zy = E::widen(row[y]);
  RowAcc acc{-__builtin_inff(), 0.0f, 0};
  int done = 0;                                         // columns [0, done) went through the 16-byte loop
  if (vec) {
    const int nvec = V / VEC;
    done = nvec * VEC;
#pragma unroll 4
    for (int i = part * SKF_WAVE + lane; i < nvec; i += ROW_WAVES * SKF_WAVE) {
      float z[VEC];
      E::load(row + (size_t)i * VEC, z);
      acc.add(z, i * VEC, zy, y);
    }
  }
#pragma unroll 4
  for (int j = done + part * SKF_WAVE + lane; j < V; j += ROW_WAVES * SKF_WAVE) {
    const float z[1] = {E::widen(row[j])};
    acc.add(z, j, zy, y);
  }
  // the lanes of a wave, then the waves of a row: max first, every sum rescaled to it
  float M = wave_max(acc.m);
  float ms = M == -__builtin_inff() ? 0.0f : M;
  float S = wave_sum(acc.s * score_exp(acc.m - ms));       // a lane without a finite entry: s == 0 and exp(-inf) == 0
  int ahead = wave_count(acc.ahead);
  if (ROW_WAVES > 1) {
    if (lane == 0) {
      sM[wave] = M;
      sS[wave] = S;
      sA[wave] = ahead;
    }
    __syncthreads();
    if (!writer) return;
    M = sM[0];
#pragma unroll
    for (int w = 1; w < ROW_WAVES; ++w) M = fmaxf(M, sM[w]);
    ms = M == -__builtin_inff() ? 0.0f : M;
    S = 0.0f;
    ahead = 0;
#pragma unroll
    for (int w = 0; w < ROW_WAVES; ++w) {
      S += sS[w] * score_exp(sM[w] - ms);
      ahead += sA[w];
    }
  }
  if (writer) {
    tok_logp[r] = (zy - M) - logf(S);                   // z_y == -inf under a finite maximum: -inf
    tok_rank[r] = ahead;
  }
}

// ---------------------------------------------------------------- 3. the sequence sum
// seq_logp[b] = ((0 + p_0) + p_1) + ..., p_t the stored tok_logp[b, t], t < n_b: one wave per sample loads 64 values at a time and
// adds them in order (a wave-uniform loop over the lanes).
__global__ __launch_bounds__(SCORE_THREADS) void score_sum_kernel(const float* __restrict__ tok_logp, const int* __restrict__ seq_len, int B,
                                                                  int T, float* __restrict__ seq_logp) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const int n = __builtin_amdgcn_readfirstlane(min(max(seq_len[b], 0), T));
  const float* row = tok_logp + (size_t)b * T;
  float sum = 0.0f;
  for (int base = 0; base < n; base += SKF_WAVE) {
    const float v = base + lane < n ? row[base + lane] : 0.0f;
    const int k = min(SKF_WAVE, n - base);
    for (int i = 0; i < k; ++i) sum += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
  }
  if (lane == 0) seq_logp[b] = sum;
}

template <bool BF16>
void score_rows_launch(const void* logits, int ld, int rows, int T, int V, const long long* target, int tgt_ld, int tgt_off,
                       const int* seq_len, float* tok_logp, int* tok_rank, hipStream_t st) {
  typedef typename ScoreElem<BF16>::T Elem;
  const int vec = ((uintptr_t)logits & 15) == 0 && ((size_t)ld * sizeof(Elem)) % 16 == 0;
  const Elem* z = (const Elem*)logits;
  if (V <= SCORE_WIDE_V)
    hipLaunchKernelGGL((score_rows_kernel<BF16, 1>), dim3(skf_cdiv(rows, SCORE_WAVES)), dim3(SCORE_THREADS), 0, st, z, ld, rows, T, V, vec,
                       target, tgt_ld, tgt_off, seq_len, tok_logp, tok_rank);
  else
    hipLaunchKernelGGL((score_rows_kernel<BF16, SCORE_WAVES>), dim3(rows), dim3(SCORE_THREADS), 0, st, z, ld, rows, T, V, vec, target,
                       tgt_ld, tgt_off, seq_len, tok_logp, tok_rank);
}

}  // namespace

extern "C" int skf_sequence_score(const void* logits, int is_bf16, int ld, int B, int T, int V, const long long* target, int tgt_ld,
                                  int tgt_off, long long eos, float* tok_logp, int* tok_rank, float* seq_logp, int* seq_len,
                                  skf_stream_t stream) {
  SKF_CHECK_ARG(logits && target && tok_logp && tok_rank && seq_logp && seq_len, "null pointer");
  SKF_CHECK_ARG(is_bf16 == 0 || is_bf16 == 1, "is_bf16 must be 0 or 1");
  SKF_CHECK_ARG(B >= 1 && T >= 1 && V >= 1, "B, T and V must be at least 1");
  SKF_CHECK_ARG((long long)B * T < (1ll << 31), "B * T must be below 2^31");
  SKF_CHECK_ARG(ld >= V, "the row pitch is shorter than a row");
  SKF_CHECK_ARG(tgt_off >= 0 && tgt_ld >= tgt_off + T, "a target row is shorter than tgt_off + T");
  SKF_CHECK_ARG(((uintptr_t)logits & (is_bf16 ? 1 : 3)) == 0, "logits must be aligned to its element");
  SKF_CHECK_ARG(((uintptr_t)target & 7) == 0, "target must be 8-byte aligned");
  SKF_CHECK_ARG(((uintptr_t)tok_logp & 3) == 0 && ((uintptr_t)tok_rank & 3) == 0 && ((uintptr_t)seq_logp & 3) == 0 && ((uintptr_t)seq_len & 3) == 0,
                "the outputs must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int rows = B * T;
  const dim3 per_sample(skf_cdiv(B, SCORE_WAVES)), block(SCORE_THREADS);
  hipLaunchKernelGGL(score_len_kernel, per_sample, block, 0, st, target, tgt_ld, tgt_off, eos, B, T, seq_len);
  if (is_bf16) score_rows_launch<true>(logits, ld, rows, T, V, target, tgt_ld, tgt_off, seq_len, tok_logp, tok_rank, st);
  else score_rows_launch<false>(logits, ld, rows, T, V, target, tgt_ld, tgt_off, seq_len, tok_logp, tok_rank, st);
  hipLaunchKernelGGL(score_sum_kernel, per_sample, block, 0, st, tok_logp, seq_len, B, T, seq_logp);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
