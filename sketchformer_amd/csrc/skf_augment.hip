// The training augmentation of continuous sketches on the device (include/skf.h: skf_sketch_augment): the loader's per-sketch
// random_scale + augment_strokes (dataloaders/distributed_stroke3.py: _augment_sketch, augment_strokes) with the same operations in
// the same order and precision, replaying the host's own uniform draws, so that the results are bit-equal to the host's.
// DESIGN.md section 3o.
//
// What decides correctness here:
//   * The draws are the host's.  The reference draws twice per sketch and once per point whether the draw is used or not, so the
//     stream depends on the lengths alone: the host draws 2 N + P doubles in one call and sketch s reads its own slice.
//   * The drop decisions hold no floating-point state: pen bits, a counter, and `u < prob` compared in float64 (a draw rounded to
//     fp32 first can land on the other side of prob).
//   * The offsets of a run of dropped points are added to the kept row before them in fp32, ONE AT A TIME in point order; summing
//     the run first rounds differently.  So the walk is sequential: one LANE owns one sketch (a chunk holds tens of thousands of
//     sketches, which is the parallelism), like the scan of skf_tokenize.hip.
//   * No contraction.  This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS) and carries the pragma below as well: the
//     scale factor's multiply and add, and the scaling multiply followed by a merging add, are rounded one by one.
//
// Launches of skf_sketch_augment: count (per sketch: the keep bit of every point, the number of kept rows) -> offsets (the shared
// scan of skf_ragged.hip) -> write (per sketch: the compacted rows with the merged sums).  No atomics; every output element
// has one writer per launch and the launches are ordered by the stream.
#include "skf_ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 64;           // one wave per workgroup, like the encode scan: 70k sketches are ~1100 waves

struct AugmentParams {
  const float* flat;            // (P, 3) rows (dx, dy, pen)
  const long long* offsets;     // N + 1
  const double* rnd;            // 2 N + P: per sketch ux, uy, then one draw per point
  long long P;
  int N, clamp;
  double scale_factor, prob;
  float* out_flat;              // (P, 3) capacity
  long long* out_offsets;       // N + 1
  int* counts;                  // workspace: kept rows per sketch
  unsigned char* keep;          // workspace: per point, 1 = kept, 0 = merged into the kept row before it
};

// Walk 1.  augment_strokes' loop without its arithmetic: prev is the pen of the last kept row (1 before the first point), count
// the distance to the last point where either pen was 1; a point goes when pen == 0, prev == 0, count > 2 and its draw is below
// prob.  A dropped point has pen 0 and so has the row it is merged into: prev only changes at kept points.
__global__ __launch_bounds__(AUG_THREADS) void augment_count_kernel(AugmentParams q) {
  const long long s = (long long)blockIdx.x * AUG_THREADS + threadIdx.x;
  if (s >= q.N) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  const float* rows = q.flat + 3 * (size_t)beg;
  const double* u = q.rnd + (size_t)beg + 2 * (size_t)s + 2;                   // behind the sketch's two scale draws
  unsigned char* keep = q.keep + (size_t)beg;
  float prev = 1.0f;
  int count = 0, kept = 0;
  for (int t = 0; t < n; ++t) {
    const float pen = skf_sketch_clamp(rows[3 * t + 2], q.clamp);
    count = (pen == 1.0f || prev == 1.0f) ? 0 : count + 1;
    const bool drop = pen == 0.0f && prev == 0.0f && count > 2 && u[t] < q.prob;
    keep[t] = drop ? 0 : 1;
    if (!drop) { prev = pen; ++kept; }
  }
  q.counts[s] = kept;
}

// Walk 2.  fx, fy in float64 and rounded once; every point scaled in fp32; a kept point opens a row, a dropped point is added to
// the open row, one fp32 add per point in point order; the row is stored when the next one opens.
__global__ __launch_bounds__(AUG_THREADS) void augment_write_kernel(AugmentParams q) {
  const long long s = (long long)blockIdx.x * AUG_THREADS + threadIdx.x;
  if (s >= q.N) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  if (n == 0) return;
  const float* rows = q.flat + 3 * (size_t)beg;
  const unsigned char* keep = q.keep + (size_t)beg;
  const double* u = q.rnd + (size_t)beg + 2 * (size_t)s;
  const float fx = (float)(((u[0] - 0.5) * 2.0) * q.scale_factor + 1.0);
  const float fy = (float)(((u[1] - 0.5) * 2.0) * q.scale_factor + 1.0);
  long long o = q.out_offsets[s];
  float ax = 0.0f, ay = 0.0f, ap = 0.0f;
  bool open = false;
  for (int t = 0; t < n; ++t) {
    const float x = skf_sketch_clamp(rows[3 * t], q.clamp) * fx;
    const float y = skf_sketch_clamp(rows[3 * t + 1], q.clamp) * fy;
    if (keep[t]) {
      // (o < P: offsets that overlap - the caller's error - would count more rows than out_flat holds)
      if (open && o < q.P) { float* r = q.out_flat + 3 * (size_t)o; r[0] = ax; r[1] = ay; r[2] = ap; }
      if (open) ++o;
      ax = x; ay = y; ap = skf_sketch_clamp(rows[3 * t + 2], q.clamp);
      open = true;
    } else {
      ax = ax + x; ay = ay + y;
    }
  }
  if (open && o < q.P) { float* r = q.out_flat + 3 * (size_t)o; r[0] = ax; r[1] = ay; r[2] = ap; }
}

// the workspace of skf_sketch_augment; returns its size
size_t augment_carve(void* ws, long long P, int N, AugmentParams& q) {
  SkfWsCarver c(ws);
  q.counts = c.take<int>(N); q.keep = c.take<unsigned char>(P);
  return c.used;
}

}  // namespace

extern "C" size_t skf_sketch_augment_workspace_bytes(long long P, int N) {
  if (P < 1 || P >= (1ll << 31) || N < 1) return 0;
  AugmentParams q;
  return augment_carve(nullptr, P, N, q);
}

extern "C" int skf_sketch_augment(const float* flat, long long P, const long long* offsets, int N, const double* rnd,
                                  double scale_factor, double prob, unsigned flags, float* out_flat, long long* out_offsets,
                                  void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(flat, P, offsets, N, workspace, workspace_bytes, skf_sketch_augment_workspace_bytes(P, N));
  SKF_CHECK_ARG(rnd && out_flat && out_offsets, "null pointer");
  SKF_CHECK_ARG(prob > 0.0 && prob <= 1.0, "prob must be in (0, 1]");
  SKF_CHECK_ARG(scale_factor >= 0.0 && scale_factor < 1.0, "scale_factor must be in [0, 1)");
  SKF_CHECK_ARG((flags & ~(unsigned)SKF_AUGMENT_CLAMP) == 0, "unknown flag");
  SKF_CHECK_ARG(((uintptr_t)rnd & 7) == 0 && ((uintptr_t)out_flat & 3) == 0 && ((uintptr_t)out_offsets & 7) == 0,
                "rnd, out_flat, out_offsets must be aligned to their element");
  hipStream_t st = (hipStream_t)stream;
  AugmentParams q;
  q.flat = flat; q.offsets = offsets; q.rnd = rnd; q.P = P; q.N = N; q.clamp = (flags & SKF_AUGMENT_CLAMP) ? 1 : 0;
  q.scale_factor = scale_factor; q.prob = prob; q.out_flat = out_flat; q.out_offsets = out_offsets;
  augment_carve(workspace, P, N, q);

  hipLaunchKernelGGL(augment_count_kernel, dim3(skf_cdiv(N, AUG_THREADS)), dim3(AUG_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  skf_counts_to_offsets_launch(q.counts, N, out_offsets, st);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(augment_write_kernel, dim3(skf_cdiv(N, AUG_THREADS)), dim3(AUG_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
