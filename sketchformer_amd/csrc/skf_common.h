// Shared device/host helpers for the sketchformer_amd HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/skf.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define SKF_WAVE 64

// The shipped library reads NO environment variable and keeps no configuration state (include/skf.h).
void skf_set_error(const char* fmt, ...);

#define SKF_CHECK_ARG(cond, msg)                                   \
  do {                                                             \
    if (!(cond)) {                                                 \
      skf_set_error("%s: %s (%s)", __func__, msg, #cond);          \
      return SKF_EINVAL;                                           \
    }                                                              \
  } while (0)

#define SKF_LAUNCH_CHECK()                                          \
  do {                                                              \
    hipError_t e__ = hipGetLastError();                             \
    if (e__ != hipSuccess) {                                        \
      skf_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e__)); \
      return SKF_EHIP;                                              \
    }                                                               \
  } while (0)

#define SKF_HIP(call)                                               \
  do {                                                              \
    hipError_t e__ = (call);                                        \
    if (e__ != hipSuccess) {                                        \
      skf_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e__)); \
      return SKF_EHIP;                                              \
    }                                                               \
  } while (0)

// Optional per-launch timing (HIP events on the launch stream), used by bench.py for the
// roofline figures.  Inactive (one branch) unless skf_profiler_enable(1) was called.
struct SkfProfScope {
  SkfProfScope(hipStream_t st, const char* tag, double flops, double bytes);
  ~SkfProfScope();
  // Work the launch actually performs when it walks a live-row / live-tile list or skips masked tiles (flops, bytes are the
  // dense figures).  Call only when active(): the fractions below synchronise the device and read the lists back.
  void done(double flops_done, double bytes_done);
  bool active() const { return idx_ >= 0; }
  hipStream_t st_;
  int idx_;
};
// Profiling only (both synchronise the device): live share of a {n_live, n_total, ...} list (skf_row_blocks.hip), and the
// share of (query tile, key tile) pairs an attention launch visits: per sample the query tiles below q_live[b] (all when
// null), the key tiles up to the last un-padded key (all when the mask is null) and, with a look-ahead mask that may be
// skipped (key 0 visible), only key tiles kt <= qt.
double skf_prof_list_fraction(const int* list);
double skf_prof_attention_fraction(const unsigned char* key_mask, int mask_ld, int causal, int B, int Lq, int Lk,
                                   const int* q_live, int qtile, int ktile);

// Launchers that the step orchestrator (skf_model*.hip) calls and include/skf.h does not declare.  skf_optimizer.hip: the Adam sweep;
// advance != 0 = the sweep of a whole step, which also performs skf_step_epilogue's increment.  skf_rowops.hip: the pooling scorer's /
// the expander's backward without their column sums (the partials are left for the batched reduction), and the staging launch.
int skf_adam_step_launch(float* w, const float* g, float* m, float* v, size_t n, void* step_state, float grad_scale, float beta1, float beta2,
                         float eps, int advance, hipStream_t stream);
int skf_pool_bwd_partials(float* u_inout_dpre, const float* Vw, const float* x, const float* a, const float* demb, int B, int L, int U, int d,
                          float* dx, float* dV_part, hipStream_t s);
int skf_expander_bwd_partials(const float* dpre, const float* emb, const float* w, int B, int L, int d, float* demb, int demb_accumulate,
                              float* p1, float* p2, hipStream_t s);
int skf_stage_inputs_launch(const void* inp, void* dinp, const void* tar, void* dtar, size_t row, size_t src_row, size_t copy, int batch,
                            const void* labels, void* dlabels, hipStream_t st, unsigned char* emask = nullptr, unsigned char* dmask = nullptr,
                            int mask_L = 0);
// skf_ragged.hip: out_offsets[0] = 0, out_offsets[i + 1] = counts[0] + .. + counts[i]; one launch, the caller checks it
// (SKF_LAUNCH_CHECK).
int skf_counts_to_offsets_launch(const int* counts, int N, long long* out_offsets, hipStream_t stream);

static inline int skf_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Workspaces are cut into regions that each start on a 256-byte boundary.  An operation states its layout ONCE, as a function that
// takes its regions from a carver in order; its *_workspace_bytes runs that function on a null base and returns `used`, its entry
// point runs it on the caller's buffer.
constexpr size_t skf_ws_align(size_t n) { return (n + 255) & ~(size_t)255; }
struct SkfWsCarver {
  uintptr_t base;
  size_t used = 0;
  explicit SkfWsCarver(void* ws) : base((uintptr_t)ws) {}
  template <class T> T* take(size_t count) { T* p = (T*)(base + used); used += skf_ws_align(count * sizeof(T)); return p; }
};

// An event that means "everything this stream was given so far is complete" costs the stream ~5 us as a packet of its own
// (hipEventRecord) and ~1.3 us attached to the kernel launch in front of it as that command's completion signal (hipExtLaunchKernelGGL's
// stop event; tools/micro/event_cost.hip, profiles/r06c_event_cost.txt: 25.4 vs 21.7 us per iteration against 20.4 without any event).
//
// The attach protocol, all of it:
//  - PARK.  A caller that wants event E behind the LAST launch of the calls it is about to make opens an SkfTailScope(E) around them
//    and asks scope.attached() afterwards: true = E is that launch's completion signal, false = nothing carries E and the caller
//    records it (hipEventRecord) as before.  The scope restores what the slot held before on every way out, so an early return or an
//    error can neither leak E into a later launch nor lose an outer scope's event.  SkfTailScope(nullptr) only shields the calls
//    inside it: launches on ANOTHER stream (the side stream's weight gradients) must never pick up an event parked for this one.
//  - ATTACH.  Only SKF_LAUNCH_TAIL attaches, and it says so (slot.attached); nobody infers it from an empty slot.  A launch site may
//    use SKF_LAUNCH_TAIL only where it is the last launch of every entry point that reaches it with an event parked (each site
//    carries a comment that names its parkers); a site that is not simply launches with hipLaunchKernelGGL and the event is recorded.
//  - CHAIN.  A launcher that issues several SKF_LAUNCH_TAIL launches takes the event out at entry (skf_tail_defer) and puts it back
//    in front of its final launch (skf_tail_resume).  A chain that fails midway never puts it back: the event stays un-attached.
// Nothing is parked while a step is captured into a hipGraph (the orchestrator's with_tail_event checks); the slot is per host thread.
struct SkfTailSlot {
  hipEvent_t event = nullptr;      // parked for this thread's next SKF_LAUNCH_TAIL launch
  bool attached = false;           // that launch has taken it
};
extern thread_local SkfTailSlot skf_tls_tail;      // (defined in skf_model.hip; named in this header only)
struct SkfTailScope {
  explicit SkfTailScope(hipEvent_t e) : saved_(skf_tls_tail) { skf_tls_tail = SkfTailSlot{e, false}; }
  ~SkfTailScope() { skf_tls_tail = saved_; }
  SkfTailScope(const SkfTailScope&) = delete;
  SkfTailScope& operator=(const SkfTailScope&) = delete;
  bool attached() const { return skf_tls_tail.attached; }
 private:
  SkfTailSlot saved_;
};
inline hipEvent_t skf_tail_defer() { hipEvent_t e = skf_tls_tail.event; skf_tls_tail.event = nullptr; return e; }
inline void skf_tail_resume(hipEvent_t e) { skf_tls_tail.event = e; }
inline hipEvent_t skf_tail_attach() {      // SKF_LAUNCH_TAIL only
  hipEvent_t e = skf_tls_tail.event;
  if (e) skf_tls_tail = SkfTailSlot{nullptr, true};
  return e;
}
#define SKF_LAUNCH_TAIL(kernel, grid, block, smem, stream, ...)                                        \
  do {                                                                                                 \
    if (hipEvent_t ev__ = skf_tail_attach()) {                                                         \
      hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, nullptr, ev__, 0, __VA_ARGS__);         \
    } else {                                                                                           \
      hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                              \
    }                                                                                                  \
  } while (0)

// "Once per DEVICE" guard for hipFuncSetAttribute (the attribute belongs to the (function, device) pair; one process may drive
// several GPUs, one host thread each):
//     static SkfOncePerDevice once;  if (once.needed()) { SKF_HIP(hipFuncSetAttribute(...)); once.mark(); }
// The bit is set AFTER the attribute call succeeded (a second host thread on the same device either sees the bit and finds the
// attribute applied, or sets the attribute again itself - idempotent) and with an atomic OR (threads of different devices share the word).
struct SkfOncePerDevice {
  unsigned long long done = 0;
  static int device() {
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) ? dev : -1;
  }
  bool needed() const {
    const int dev = device();
    return dev < 0 || !((__atomic_load_n(&done, __ATOMIC_ACQUIRE) >> dev) & 1ull);      // unknown device: always set
  }
  void mark() {
    const int dev = device();
    if (dev >= 0) __atomic_fetch_or(&done, 1ull << dev, __ATOMIC_RELEASE);
  }
};

// ---------------------------------------------------------------- device
// Bijective XCD-aware remap of a 1-D grid: block b runs on XCD b % 8 (observed dispatch order), so giving
// every XCD a CONTIGUOUS range of logical ids keeps workgroups that share operand panels on one L2.
__device__ __forceinline__ int skf_xcd_remap(int orig, int nwg) {
  const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}
// Numbering of work items (group g, part w) whose cost depends on the PART with a period that divides the dispatcher's own.
// Consecutive workgroups of an XCD are handed to its 4 shader engines in turn and a workgroup only ever runs on the 8 CUs of the
// engine it was handed to, so with 4 parts per group and the part as the fastest index every heavy part (the one live 128-key block
// of a padded sample, the last query block under the look-ahead mask) queues on the same quarter of the chip and the launch takes
// as long as if all parts were heavy (measured, bf16 dK/dV pass, B 128 / H 8 / L 512: 8 live keys of 512 223 us against 236 us
// full-length, 111 us with this numbering; profiles/r05n_bf16_attn_dispatch.txt).  Here: chunks of 32 groups, part-major inside a
// chunk, so 32 consecutive workgroups carry the same part (part 0 first) and the parts of a group stay close enough in time to
// share the L2.
__device__ __forceinline__ void skf_part_major(int lid, int ngroups, int nparts, int* g, int* w) {
  constexpr int G = 32;
  const int chunk = lid / (G * nparts), j = lid - chunk * G * nparts;
  const int gc = min(G, ngroups - chunk * G);
  *w = j / gc;
  *g = chunk * G + j - *w * gc;
}
// The other way round: workgroups whose cost is known per SAMPLE (padded batches: one workgroup per (sample, head)).  Given the
// samples sorted by cost (heaviest first), workgroup `bid` (-> XCD bid % 8, arrival i = bid / 8 in that XCD -> engine i % 4) takes head
// i % H of the sample with rank (bid % 8) + 8 * (i / H): the sorted list is DEALT over the XCDs, heaviest first, and the heads of a
// sample stay on one XCD, spread over its engines - every XCD and every engine gets the same mix of lengths, and an XCD reads whole
// activation rows (its heads' slices side by side: with the heads of a row on eight XCDs each L2 saw one 128-byte slice per KB and the
// bf16 dQ pass ran 27 % slower).  Returns rank * H + head; needs B % 8 == 0 (the caller checks).
__device__ __forceinline__ int skf_deal_rank(int bid, int H) {
  const int x = bid & 7, i = bid >> 3, m = i / H;
  return (x + 8 * m) * H + (i - m * H);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// The fp64 sum over a 256-thread block, sRed = 4 doubles of LDS; every thread gets the sum.  The order (butterfly, then waves
// 0..3) is fixed: it is part of the bit-equality of the k-means and t-SNE results.
__device__ __forceinline__ double block_sum(double v, double* sRed) {
  v = wave_sum(v);
  __syncthreads();                                // sRed of the previous use is read
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// (x, y) -> P dwords; dword q = bf16 piece q of x in the low half, of y in the high half.  Pieces are the top 16 bits
// of the running remainder (truncation), remainders are exact: x = x0 + x1 + x2 for every finite fp32 (24 significand
// bits = 3 x 8).  The remainder x - x_q is one v_dot2c_f32_bf16 (x += piece . (-1, 0)) instead of a mask and a subtract.
typedef __bf16 skf_bf16x2 __attribute__((ext_vector_type(2)));
// the (-1, 0) / (0, -1) selectors of the remainder dot products, kept opaque in SGPRs (folded into the inline constant
// "-1.0" the instruction subtracted the wrong half on gfx950).  Create ONCE per kernel: the asm is not hoisted.
struct SkfSplitSel { unsigned lo, hi; };
__device__ __forceinline__ SkfSplitSel skf_split_sel() {
  SkfSplitSel r{0x0000bf80u, 0xbf800000u};
  asm volatile("" : "+s"(r.lo), "+s"(r.hi));
  return r;
}
template <int P>
__device__ __forceinline__ void skf_split2(float x, float y, unsigned (&out)[P], const SkfSplitSel& sel) {
#pragma unroll
  for (int q = 0; q < P; ++q) {
    out[q] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, x), 0x07060302u);   // (y & 0xffff0000) | (x >> 16)
    if (q + 1 < P) {
      const skf_bf16x2 pc = __builtin_bit_cast(skf_bf16x2, out[q]);
      x = __builtin_amdgcn_fdot2_f32_bf16(pc, __builtin_bit_cast(skf_bf16x2, sel.lo), x, false);
      y = __builtin_amdgcn_fdot2_f32_bf16(pc, __builtin_bit_cast(skf_bf16x2, sel.hi), y, false);
    }
  }
}

// Counter-based dropout RNG: one 32-bit hash per element, keyed on
// (key = f(seed, step), site, flat element index).  Deterministic, stateless,
// identical on host (skf_dropout_keep_mask) and device.
__host__ __device__ __forceinline__ uint32_t skf_hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
// Counter-based uniform of the sampled decode: draw `step` of the caller's stream `stream_id` under `seed`, three hash rounds,
// as 24 bits n (the uniform is n * 2^-24, in [0, 1)).  Stateless; identical on host (skf_sample_uniform) and device.
__host__ __device__ __forceinline__ uint32_t skf_sample_bits24(uint32_t seed, uint32_t stream_id, uint32_t step) {
  uint32_t h = skf_hash32(seed + 0x243f6a88U);
  h = skf_hash32(h ^ (stream_id * 0x9e3779b1U));
  h = skf_hash32(h + step * 0x85ebca6bU);
  return h >> 8;
}
__host__ __device__ __forceinline__ float skf_sample_uniform01(uint32_t seed, uint32_t stream_id, uint32_t step) {
  return (float)skf_sample_bits24(seed, stream_id, step) * (1.0f / 16777216.0f);
}
__host__ __device__ __forceinline__ uint32_t skf_site_key(uint32_t key, uint32_t site) {
  return skf_hash32(key ^ (0x9e3779b9U * (site + 1)));
}
constexpr uint32_t kSkfKeepStride = 0x9e3779b1U;   // hash argument of element idx = idx * kSkfKeepStride + site_key
// the same decision from the hash argument itself: kernels that walk idx in fixed steps add multiples of kSkfKeepStride
// instead of multiplying per element (v_mul_lo_u32 is a quarter-rate instruction)
__host__ __device__ __forceinline__ bool skf_keep_arg(uint32_t arg, uint32_t thresh) { return skf_hash32(arg) >= thresh; }
__host__ __device__ __forceinline__ bool skf_keep(uint32_t site_key, uint32_t idx, uint32_t thresh) {
  // keep iff u >= rate  (tf.nn.dropout: random_uniform >= rate)
  return skf_keep_arg(idx * kSkfKeepStride + site_key, thresh);
}
__host__ __device__ __forceinline__ uint32_t skf_drop_thresh(float rate) {
  double t = (double)rate * 4294967296.0;
  return t >= 4294967295.0 ? 0xffffffffU : (uint32_t)t;
}

// Per-step scalars that live in device memory so a captured hipGraph can be
// replayed: written by the step-prologue kernel, read by dropout sites / Adam.
struct SkfStepState {
  long long iterations;   // optimizer.iterations (pre-increment value used this step)
  float lr;               // schedule(iterations)
  float alpha;            // lr * sqrt(1-b2^t)/(1-b1^t)
  uint32_t drop_key;      // hash(seed, iterations) at micro == 0, hash(seed, iterations, micro) behind it (skf_drop_key)
  uint32_t micro;         // micro-batches already summed into the open optimizer step (gradient accumulation, skf_accum.hip); 0 without it
};
static_assert(sizeof(SkfStepState) == 24, "step state layout (include/skf.h, ops.read_step_state)");
// The dropout key of micro-step `micro` of optimizer step `it`.  micro == 0 is the key every step had before accumulation existed;
// micro = j > 0 hashes j (under a constant of its own) INTO that key: a third hash round over (seed, iterations, j), not a shift of
// `iterations` - key(it, j) and key(it + j, 0) are unrelated words, so no micro-step redraws the masks of a later optimizer step.
__host__ __device__ __forceinline__ uint32_t skf_drop_key(uint32_t seed, long long it, uint32_t micro) {
  const uint32_t key = skf_hash32(seed ^ skf_hash32((uint32_t)it + 0x632be5abU));
  return micro == 0 ? key : skf_hash32(key ^ skf_hash32(micro + 0x5bd1e995U));
}
