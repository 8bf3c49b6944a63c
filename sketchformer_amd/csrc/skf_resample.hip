// Arc-length resampling of polylines on the device (include/skf.h: skf_polyline_resample_count / _emit / _n), bit-equal to the
// host restatement of tests/resample_reference.py.  DESIGN.md section 3t.
//
// What decides correctness here:
//   * The rule is built so that the order of evaluation is free.  A segment's length is c = sqrtf(dx * dx + dy * dy) in fp32, every
//     operation rounded on its own, and is then FIXED to q = (int64) rint((double) c * 2^16); the arc-length table C is the integer
//     running sum of q, so a wave scan with a carry from tile to tile and a sequential host sum agree exactly.  Targets are integers
//     too (m * s, or floor(m * total / (n_out - 1))), the segment of a target is found by comparing integers, and a sample is three
//     fp64 operations on exact inputs: u = (T - C_i) / q_i, x = x_i + u * (x_{i+1} - x_i), each rounded on its own, then one rounding
//     to fp32.  This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS) and carries the pragma below as well.
//   * Measure launch: one wavefront per polyline walks it in tiles of 64 points, writes C for every point to the workspace (C of
//     the polyline's first point is 0) and the polyline's number of output rows to counts.  The shared counts -> offsets scan
//     (skf_ragged.hip) follows.
//   * Emit launch: one wavefront per polyline, every lane owns one output row per tile of 64 rows, consecutive lanes consecutive
//     targets: the 8-byte stores of a tile are one contiguous 512-byte run.  A lane finds its segment by binary search over the
//     polyline's slice of C; the targets are independent, so nothing is carried between lanes or tiles.
//   * Every range of input rows is clamped to [0, P] (skf_ragged_range) and every store to the capacity the caller states; an offset
//     is never an index.  A polyline's walk stops where its rows leave the capacity, so its cost is bounded by what can be written.
// No atomics, no allocation, no host synchronisation; every output element has one writer.
#include "skf_ragged.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RS_WAVES = 4;               // polylines per workgroup, one wave each (no LDS, no workgroup barrier)
constexpr int RS_THREADS = 64 * RS_WAVES;
constexpr double RS_UNIT = 65536.0;       // arc lengths are integers in units of 2^-16

struct ResampleParams {
  const float* xy;              // (P, 2) absolute points, ldp floats from row to row
  long long ldp, P;
  const long long* offsets;     // S + 1
  int S;
  long long step;               // spacing mode: rint(spacing * 2^16) >= 1
  int n_out;                    // count mode: rows per polyline
  const long long* out_offsets; // spacing mode, S + 1: what the scan wrote
  float* out_xy;                // spacing mode (out_rows, 2); count mode (S, n_out, 2)
  long long out_rows;
  int* counts;                  // workspace, S: output rows per polyline
  long long* C;                 // workspace, P: the arc-length table, C[beg] = 0 for every polyline
};

// the number of output rows of a polyline of arc length total at spacing step: ceil(total / step) + 1, at most INT_MAX
__device__ __forceinline__ int resample_rows(long long total, long long step) {
  if (total <= 0) return 1;
  const long long full = total / step + (total % step != 0 ? 1 : 0);
  return full >= (long long)INT_MAX ? INT_MAX : (int)(full + 1);
}

__global__ __launch_bounds__(RS_THREADS) void resample_measure_kernel(ResampleParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * RS_WAVES + wave;
  if (s >= q.S) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  if (n == 0) {
    if (lane == 0) q.counts[s] = 0;
    return;
  }
  const float* src = q.xy + (size_t)beg * q.ldp;
  long long* C = q.C + (size_t)beg;
  if (lane == 0) C[0] = 0;
  long long carry = 0;
  for (long long i0 = 0; i0 < n - 1; i0 += 64) {                               // (the trip count is the same for every lane)
    const long long i = i0 + lane;                                             // the segment from point i to point i + 1
    long long v = 0;
    if (i < n - 1) {
      const float dx = src[(i + 1) * q.ldp] - src[i * q.ldp];
      const float dy = src[(i + 1) * q.ldp + 1] - src[i * q.ldp + 1];
      const float c = sqrtf(dx * dx + dy * dy);
      v = (long long)rint((double)c * RS_UNIT);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    if (i < n - 1) C[i + 1] = carry + v;
    carry += __shfl(v, 63, 64);
  }
  if (lane == 0) q.counts[s] = resample_rows(carry, q.step);
}

// The sample at target T, 0 <= T < C[n - 1], of the polyline src (n >= 2 points) with the table C.
__device__ __forceinline__ float2 resample_at(const float* src, long long ldp, const long long* C, int n, long long T) {
  int lo = 0, hi = n - 1;                                                      // C[lo] <= T < C[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (C[mid] <= T) lo = mid; else hi = mid;
  }
  const long long c0 = C[lo];
  const double u = (double)(T - c0) / (double)(C[lo + 1] - c0);
  const double x0 = (double)src[lo * ldp], y0 = (double)src[lo * ldp + 1];
  const double x1 = (double)src[(lo + 1) * ldp], y1 = (double)src[(lo + 1) * ldp + 1];
  return make_float2((float)(x0 + u * (x1 - x0)), (float)(y0 + u * (y1 - y0)));
}

__global__ __launch_bounds__(RS_THREADS) void resample_emit_kernel(ResampleParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * RS_WAVES + wave;
  if (s >= q.S) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  if (n == 0) return;
  const float* src = q.xy + (size_t)beg * q.ldp;
  const long long* C = q.C + (size_t)beg;
  const int rows = resample_rows(n >= 2 ? C[n - 1] : 0, q.step);                // (a single point has no table to trust)
  const long long o = q.out_offsets[s];
  float2* out = (float2*)q.out_xy;
  // rows o + m, m = 0 .. rows - 1; only those inside [0, out_rows) are looked at
  for (long long m0 = o < 0 ? ((-o) & ~63ll) : 0; m0 < rows && o + m0 < q.out_rows; m0 += 64) {
    const long long m = m0 + lane, row = o + m;
    if (m >= rows || row < 0 || row >= q.out_rows) continue;
    if (m == rows - 1) out[row] = make_float2(src[(long long)(n - 1) * q.ldp], src[(long long)(n - 1) * q.ldp + 1]);
    else out[row] = resample_at(src, q.ldp, C, n, m * q.step);                 // m < ceil(total / step): m * step < total
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_emit_n_kernel(ResampleParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * RS_WAVES + wave;
  if (s >= q.S) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  float2* out = (float2*)q.out_xy + (size_t)s * (size_t)q.n_out;
  const float* src = q.xy + (size_t)beg * q.ldp;
  const long long* C = q.C + (size_t)beg;
  const long long total = n >= 2 ? C[n - 1] : 0;
  const long long last = q.n_out - 1;
  const long long a = total / last, r = total % last;
  for (int m = lane; m < q.n_out; m += 64) {
    float2 v = make_float2(0.0f, 0.0f);                                        // an empty polyline is the single point (0, 0)
    if (n > 0 && total <= 0) v = make_float2(src[0], src[1]);
    else if (n > 0 && m == last) v = make_float2(src[(long long)(n - 1) * q.ldp], src[(long long)(n - 1) * q.ldp + 1]);
    else if (n > 0) v = resample_at(src, q.ldp, C, n, m * a + (m * r) / last);   // floor(m * total / last) < total
    out[m] = v;
  }
}

size_t resample_carve(void* ws, long long P, int S, ResampleParams& q) {
  SkfWsCarver c(ws);
  q.counts = c.take<int>(S); q.C = c.take<long long>(P);
  return c.used;
}

// rint(spacing * 2^16) as an integer, 0 when the spacing is refused
long long resample_step(double spacing) {
  if (!(spacing > 0.0) || !(spacing < 7.0e13)) return 0;                       // (false for a NaN); the step stays below 2^62
  return (long long)rint(spacing * RS_UNIT);
}

}  // namespace

extern "C" size_t skf_polyline_resample_workspace_bytes(long long P, int S) {
  if (P < 1 || P >= (1ll << 31) || S < 1) return 0;
  ResampleParams q;
  return resample_carve(nullptr, P, S, q);
}

extern "C" int skf_polyline_resample_count(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, double spacing,
                                           long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(xy, P, stroke_offsets, S, workspace, workspace_bytes, skf_polyline_resample_workspace_bytes(P, S));
  SKF_CHECK_ARG(out_offsets && ((uintptr_t)out_offsets & 7) == 0, "out_offsets must be an 8-byte aligned pointer");
  SKF_CHECK_ARG(ldp >= 2, "ldp must be at least 2");
  SKF_CHECK_ARG(resample_step(spacing) >= 1, "spacing must be finite, below 7e13, with rint(spacing * 2^16) >= 1");
  hipStream_t st = (hipStream_t)stream;
  ResampleParams q = {};
  q.xy = xy; q.ldp = ldp; q.P = P; q.offsets = stroke_offsets; q.S = S; q.step = resample_step(spacing);
  resample_carve(workspace, P, S, q);
  hipLaunchKernelGGL(resample_measure_kernel, dim3(skf_cdiv(S, RS_WAVES)), dim3(RS_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  skf_counts_to_offsets_launch(q.counts, S, out_offsets, st);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_polyline_resample_emit(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, double spacing,
                                          const long long* out_offsets, float* out_xy, long long out_rows, void* workspace,
                                          size_t workspace_bytes, skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(xy, P, stroke_offsets, S, workspace, workspace_bytes, skf_polyline_resample_workspace_bytes(P, S));
  SKF_CHECK_ARG(out_offsets && out_xy && ((uintptr_t)out_offsets & 7) == 0 && ((uintptr_t)out_xy & 7) == 0,
                "out_offsets and out_xy must be 8-byte aligned pointers");
  SKF_CHECK_ARG(ldp >= 2, "ldp must be at least 2");
  SKF_CHECK_ARG(resample_step(spacing) >= 1, "spacing must be finite, below 7e13, with rint(spacing * 2^16) >= 1");
  SKF_CHECK_ARG(out_rows >= 1 && out_rows < (1ll << 31), "out_rows must be in [1, 2^31)");
  ResampleParams q = {};
  q.xy = xy; q.ldp = ldp; q.P = P; q.offsets = stroke_offsets; q.S = S; q.step = resample_step(spacing);
  q.out_offsets = out_offsets; q.out_xy = out_xy; q.out_rows = out_rows;
  resample_carve(workspace, P, S, q);
  hipLaunchKernelGGL(resample_emit_kernel, dim3(skf_cdiv(S, RS_WAVES)), dim3(RS_THREADS), 0, (hipStream_t)stream, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_polyline_resample_n(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, int n_out,
                                       float* out_xy, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(xy, P, stroke_offsets, S, workspace, workspace_bytes, skf_polyline_resample_workspace_bytes(P, S));
  SKF_CHECK_ARG(out_xy && ((uintptr_t)out_xy & 7) == 0, "out_xy must be an 8-byte aligned pointer");
  SKF_CHECK_ARG(ldp >= 2, "ldp must be at least 2");
  SKF_CHECK_ARG(n_out >= 2 && n_out <= SKF_RESAMPLE_MAX_N, "n_out must be in [2, 65536]");
  hipStream_t st = (hipStream_t)stream;
  ResampleParams q = {};
  q.xy = xy; q.ldp = ldp; q.P = P; q.offsets = stroke_offsets; q.S = S; q.step = 1; q.n_out = n_out; q.out_xy = out_xy;
  resample_carve(workspace, P, S, q);
  hipLaunchKernelGGL(resample_measure_kernel, dim3(skf_cdiv(S, RS_WAVES)), dim3(RS_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(resample_emit_n_kernel, dim3(skf_cdiv(S, RS_WAVES)), dim3(RS_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
