// The counts -> offsets scan of the ragged pipelines (skf_common.h: skf_counts_to_offsets_launch): the middle launch of
// skf_sketch_augment and skf_stroke3_simplify, between the walk that counts a sketch's kept rows and the walk that writes them.
// Integer sums only.
#include "skf_common.h"

namespace {

constexpr int OFFS_THREADS = 1024;        // the block width of the offsets scan: N counts go through in tiles of this many

// out_offsets[0] = 0, out_offsets[i + 1] = counts[0] + .. + counts[i].  One block walks the counts in tiles of OFFS_THREADS with a
// carry: a shuffle scan inside every wave, the waves' totals through LDS.  Integer sums: the order is free.
__global__ __launch_bounds__(OFFS_THREADS) void counts_to_offsets_kernel(const int* __restrict__ counts, int N,
                                                                          long long* __restrict__ out_offsets) {
  __shared__ long long wave_total[OFFS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (long long base = 0; base < N; base += OFFS_THREADS) {                   // (the trip count is the same for every thread)
    const long long i = base + threadIdx.x;
    long long v = i < N ? (long long)counts[i] : 0;
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    if (lane == 63) wave_total[wave] = v;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < OFFS_THREADS / 64; ++w) {
      const long long t = wave_total[w];
      if (w < wave) before += t;
      total += t;
    }
    if (i < N) out_offsets[i + 1] = carry + before + v;
    carry += total;
    __syncthreads();                                                           // wave_total is rewritten by the next tile
  }
  if (threadIdx.x == 0) out_offsets[0] = 0;
}

}  // namespace

int skf_counts_to_offsets_launch(const int* counts, int N, long long* out_offsets, hipStream_t stream) {
  hipLaunchKernelGGL(counts_to_offsets_kernel, dim3(1), dim3(OFFS_THREADS), 0, stream, counts, N, out_offsets);
  return SKF_OK;
}
