// Weight averaging: the exponential moving average of the flat fp32 parameter buffer (the "shadow") that evaluation and sampling
// run on, and the in-place exchange of two flat buffers that puts it where every entry point reads its weights.
//
// ema_update_kernel is tf.train.ExponentialMovingAverage / assign_moving_average without zero-debias:
//     shadow -= (shadow - w) * omd,      omd = 1 - d
// three fp32 operations per element (subtract, multiply, subtract), each rounded once - the file is built with -ffp-contract=off, a
// fused multiply-add would round the product and the last subtract together and differ from TensorFlow and from the float32 host
// restatement (tests/ema_reference.py) in the last bit.  d = decay, or with num_updates min(decay, (1 + n) / (10 + n)) for
// n = (float)iterations - TensorFlow's expression after its cast of num_updates to float32; ema_decay below is compiled for the
// device and, as skf_ema_decay_at, for the host.  Every thread derives omd itself from the device-resident step state (one uniform
// load, four scalar operations): no scalar launch in front, no host read.  skip (null = never) is the skip word of the clipped sweep: set, the launch writes nothing - a skipped step leaves the
// shadow as it leaves parameters, moments and `iterations`.  The kernel writes `shadow` alone.
//
// buffer_swap_kernel exchanges a and b as 16-byte words of integers (4-byte words in the tail): no float ever passes through an
// arithmetic unit, NaN payloads and signs survive.
//
// Launch shape of a memory-bound sweep, that of skf_accum.hip: 16-byte loads and stores, a grid of at most 2048 workgroups of 256
// threads (8 per CU) that strides over the 16-byte words, a scalar tail for n % 4.  A thread reads the words it writes before it
// writes them and no two threads share a word.  Plain vector stores only, no atomics, no workspace.  12 B of traffic per element
// for the update, 16 B for the swap.
#include "skf_common.h"

namespace {

constexpr int kEmaBlock = 256;
constexpr size_t kEmaMaxBlocks = 2048;      // 256 CUs x 8 workgroups

// fp32 throughout: the add, the add, one correctly rounded divide, the minimum
__host__ __device__ __forceinline__ float ema_decay(float decay, int num_updates, long long iterations) {
  if (!num_updates) return decay;
  const float n = (float)iterations;
  return fminf(decay, (1.0f + n) / (10.0f + n));
}

__device__ __forceinline__ float ema_step(float s, float w, float omd) {
  const float diff = s - w;
  const float delta = diff * omd;
  return s - delta;
}

__global__ __launch_bounds__(kEmaBlock) void ema_update_kernel(float* shadow, const float* w, size_t n, float decay, int num_updates,
                                                               const SkfStepState* st, const unsigned* skip) {
  if (skip != nullptr && skip[0] != 0u) return;
  const float omd = 1.0f - ema_decay(decay, num_updates, num_updates ? st->iterations : 0);
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * kEmaBlock;
  const size_t first = (size_t)blockIdx.x * kEmaBlock + threadIdx.x;
  for (size_t i = first; i < n4; i += stride) {
    float4 s = reinterpret_cast<const float4*>(shadow)[i];
    const float4 v = reinterpret_cast<const float4*>(w)[i];
    s.x = ema_step(s.x, v.x, omd); s.y = ema_step(s.y, v.y, omd); s.z = ema_step(s.z, v.z, omd); s.w = ema_step(s.w, v.w, omd);
    reinterpret_cast<float4*>(shadow)[i] = s;
  }
  for (size_t i = (n4 << 2) + first; i < n; i += stride) shadow[i] = ema_step(shadow[i], w[i], omd);
}

__global__ __launch_bounds__(kEmaBlock) void buffer_swap_kernel(uint32_t* a, uint32_t* b, size_t n) {
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * kEmaBlock;
  const size_t first = (size_t)blockIdx.x * kEmaBlock + threadIdx.x;
  for (size_t i = first; i < n4; i += stride) {
    const uint4 x = reinterpret_cast<const uint4*>(a)[i];
    const uint4 y = reinterpret_cast<const uint4*>(b)[i];
    reinterpret_cast<uint4*>(a)[i] = y;
    reinterpret_cast<uint4*>(b)[i] = x;
  }
  for (size_t i = (n4 << 2) + first; i < n; i += stride) {
    const uint32_t x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

unsigned ema_blocks(size_t n) {
  size_t blocks = ((n >> 2) + kEmaBlock - 1) / kEmaBlock;
  if (blocks > kEmaMaxBlocks) blocks = kEmaMaxBlocks;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

}  // namespace

extern "C" int skf_weight_average_validate(float decay) {
  // (both comparisons are false for NaN, one of them for either infinity)
  SKF_CHECK_ARG(decay > 0.f && decay < 1.f, "the decay of a weight average must be finite and lie in (0, 1)");
  return SKF_OK;
}

extern "C" float skf_ema_decay_at(float decay, int num_updates, long long iterations) { return ema_decay(decay, num_updates, iterations); }

extern "C" int skf_ema_update(float* shadow, const float* w, size_t n, float decay, int num_updates, const void* step_state,
                              const void* skip, skf_stream_t stream) {
  if (const int rc = skf_weight_average_validate(decay)) return rc;
  SKF_CHECK_ARG(!num_updates || step_state, "num_updates reads `iterations`: it needs the step state");
  SKF_CHECK_ARG(((uintptr_t)step_state & 7) == 0, "the step state must be 8-byte aligned");
  SKF_CHECK_ARG(((uintptr_t)skip & 3) == 0, "skip must be 4-byte aligned");
  SKF_CHECK_ARG(n == 0 || (shadow && w), "null operand");
  SKF_CHECK_ARG((((uintptr_t)shadow | (uintptr_t)w) & 15) == 0, "shadow and w must be 16-byte aligned");
  SKF_CHECK_ARG(n == 0 || shadow + n <= w || w + n <= shadow, "shadow and w must not overlap");
  if (n == 0) return SKF_OK;
  hipStream_t s = (hipStream_t)stream;
  SkfProfScope ps(s, "ema_update", 3.0 * n, 12.0 * n);
  hipLaunchKernelGGL(ema_update_kernel, dim3(ema_blocks(n)), dim3(kEmaBlock), 0, s, shadow, w, n, decay, num_updates ? 1 : 0,
                     (const SkfStepState*)step_state, (const unsigned*)skip);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_buffer_swap(float* a, float* b, size_t n, skf_stream_t stream) {
  SKF_CHECK_ARG(n == 0 || (a && b), "null operand");
  SKF_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "a and b must be 16-byte aligned");
  SKF_CHECK_ARG(n == 0 || a + n <= b || b + n <= a, "a and b must be two buffers that do not overlap");
  if (n == 0) return SKF_OK;
  hipStream_t s = (hipStream_t)stream;
  SkfProfScope ps(s, "buffer_swap", 0.0, 16.0 * n);
  hipLaunchKernelGGL(buffer_swap_kernel, dim3(ema_blocks(n)), dim3(kEmaBlock), 0, s, (uint32_t*)a, (uint32_t*)b, n);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
