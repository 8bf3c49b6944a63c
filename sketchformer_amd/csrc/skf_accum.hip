// Gradient accumulation: dst = a + b (or dst = a) over a flat fp32 buffer, and the micro-step counter of SkfStepState.
//
// k micro-batches run forward and backward, their gradients are summed here, the optimizer runs once on the sum with 1/k folded into
// its grad_scale (every loss of the model is a mean over equally sized batches: the mean of k micro-batch gradients IS the gradient of
// the batch of k * B rows).  One fp32 add per element, rounded once, nothing else: the result is the bits of a host `a + b`, inf and
// NaN pass through, and a non-finite micro-gradient poisons the sum the skip rule of the clipped sweep then sees.
//
// Launch shape of a memory-bound sweep: 16-byte loads and stores, a grid of at most 2048 workgroups of 256 threads (8 per CU) that
// strides over the 16-byte words, a scalar tail for n % 4.  Every thread reads the words it writes before it writes them and no two
// threads share a word: dst may be a or b.  Plain vector stores only, no atomics, no workspace.
//
// micro_op: one thread also updates SkfStepState::micro, the word the step prologue hashes into the dropout key (skf_common.h:
// skf_drop_key) - 1: += 1 (a micro-batch was summed), 2: = 0 (the optimizer step closes, or what is pending is dropped).  The launch
// that sums and the counter it moves are one command on the stream: a replayed step graph behind it reads the new value.
#include "skf_common.h"

namespace {

constexpr int kAccumBlock = 256;
constexpr size_t kAccumMaxBlocks = 2048;      // 256 CUs x 8 workgroups

template <bool HAS_B>
__global__ __launch_bounds__(kAccumBlock) void grad_accumulate_kernel(float* dst, const float* a, const float* b, size_t n, SkfStepState* st,
                                                                      int micro_op) {
  if (micro_op != SKF_MICRO_KEEP && blockIdx.x == 0 && threadIdx.x == 0) st->micro = micro_op == SKF_MICRO_NEXT ? st->micro + 1u : 0u;
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * kAccumBlock;
  const size_t first = (size_t)blockIdx.x * kAccumBlock + threadIdx.x;
  for (size_t i = first; i < n4; i += stride) {
    float4 v = reinterpret_cast<const float4*>(a)[i];
    if (HAS_B) {
      const float4 w = reinterpret_cast<const float4*>(b)[i];
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    reinterpret_cast<float4*>(dst)[i] = v;
  }
  for (size_t i = (n4 << 2) + first; i < n; i += stride) dst[i] = HAS_B ? a[i] + b[i] : a[i];
}

}  // namespace

extern "C" int skf_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* step_state, int micro_op,
                                   skf_stream_t stream) {
  SKF_CHECK_ARG(micro_op == SKF_MICRO_KEEP || micro_op == SKF_MICRO_NEXT || micro_op == SKF_MICRO_ZERO,
                "micro_op must be 0 (leave the counter), 1 (micro += 1) or 2 (micro = 0)");
  SKF_CHECK_ARG(micro_op == SKF_MICRO_KEEP || step_state, "a micro_op that moves the counter needs the step state");
  SKF_CHECK_ARG(((uintptr_t)step_state & 7) == 0, "the step state must be 8-byte aligned");
  SKF_CHECK_ARG(n == 0 || (dst && a), "null operand");
  SKF_CHECK_ARG((((uintptr_t)dst | (uintptr_t)a | (uintptr_t)b) & 15) == 0, "dst, a and b must be 16-byte aligned");
  if (n == 0 && micro_op == SKF_MICRO_KEEP) return SKF_OK;
  size_t blocks = ((n >> 2) + kAccumBlock - 1) / kAccumBlock;
  if (blocks > kAccumMaxBlocks) blocks = kAccumMaxBlocks;
  if (blocks < 1) blocks = 1;
  hipStream_t s = (hipStream_t)stream;
  SkfProfScope ps(s, b ? "grad_accumulate" : "grad_accumulate_copy", 0.0, (b ? 12.0 : 8.0) * n);
  if (b)
    hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3((unsigned)blocks), dim3(kAccumBlock), 0, s, dst, a, b, n, (SkfStepState*)step_state,
                       micro_op);
  else
    hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3((unsigned)blocks), dim3(kAccumBlock), 0, s, dst, a, b, n, (SkfStepState*)step_state,
                       micro_op);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
