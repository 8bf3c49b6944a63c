// Flattening of line / cubic Bezier paths to polylines on the device (include/skf.h: skf_path_flatten_count / _emit), bit-equal to
// the host restatement of tests/flatten_reference.py.  DESIGN.md section 3v.
//
// What decides correctness here:
//   * The rule is built so that the order of evaluation is free.  A segment's number of pieces n is the smallest integer in
//     [1, 4096] with (double)(n * n) * (double)(n * n) * c >= dd: n^4 is exact in fp64, the product with c is one rounding and
//     monotone in n, so a bisection here and numpy's search on the host find the same n.  The running sum of n along a subpath is
//     an integer sum: a wave scan with a carry from tile to tile and a sequential host sum agree exactly.  A row is either a copied
//     control point or six lerps a coordinate in a fixed order, every fp64 operation rounded on its own, then one rounding to
//     fp32.  This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS) and carries the pragma below as well.
//   * Count launch: one wavefront per subpath walks it in tiles of 64 segments, writes E, the inclusive running sum of n, for every
//     segment to the workspace and the subpath's number of rows (1 + the sum; 0 for an empty subpath) to counts.  The shared
//     counts -> offsets scan (skf_ragged.hip) follows.
//   * Emit launch: one wavefront per subpath, every lane owns one output row per tile of 64 rows, consecutive lanes consecutive
//     rows: the 8-byte stores of a tile are one contiguous 512-byte run.  Row 0 is the first control point; a lane finds the
//     segment of row m >= 1 by binary search over the subpath's slice of E (the smallest k with E[k] >= m); the rows are
//     independent, so nothing is carried between lanes or tiles.
//   * Every range of segments is clamped to [0, G] (skf_ragged_range) and every store to the capacity the caller states; an offset
//     is never an index.  A subpath's walk stops where its rows leave the capacity, so its cost is bounded by what can be written.
// No atomics, no allocation, no host synchronisation; every output element has one writer.
#include "skf_ragged.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int FL_WAVES = 4;               // subpaths per workgroup, one wave each (no LDS, no workgroup barrier)
constexpr int FL_THREADS = 64 * FL_WAVES;

struct FlattenParams {
  const double* ctrl;           // (G, 4, 2) control points p0 .. p3, absolute
  const int* kind;              // G: 1 = cubic, anything else = line
  long long G;
  const long long* offsets;     // S + 1
  int S;
  double c;                     // (16 / 9) * tol^2
  const long long* out_offsets; // emit, S + 1: what the scan wrote
  float* out_xy;                // emit (out_rows, 2)
  long long out_rows;
  int* counts;                  // workspace, S: output rows per subpath
  long long* E;                 // workspace, G: the inclusive running sum of n within the segment's subpath
};

// the larger of two values, a NaN if either is one (numpy's maximum; fmax would drop the NaN)
__device__ __forceinline__ double flatten_max(double a, double b) { return (a > b || a != a) ? a : b; }

// n of one segment (include/skf.h, Path flattening: pieces per segment)
__device__ __forceinline__ int flatten_pieces(const double* p, int kind, double c) {
  if (kind != 1) return 1;
  const double ax = (p[0] - 2.0 * p[2]) + p[4], ay = (p[1] - 2.0 * p[3]) + p[5];
  const double bx = (p[2] - 2.0 * p[4]) + p[6], by = (p[3] - 2.0 * p[5]) + p[7];
  const double dd = flatten_max(ax * ax + ay * ay, bx * bx + by * by);
  int lo = 1, hi = SKF_FLATTEN_MAX_N;                                          // the smallest n that passes, or MAX_N (a NaN passes nowhere)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const double n2 = (double)(mid * mid);
    if (n2 * n2 * c >= dd) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the number of rows of a subpath whose pieces add up to total (at least one segment): 1 + total, at most INT_MAX
__device__ __forceinline__ int flatten_rows(long long total) {
  return total >= (long long)INT_MAX - 1 ? INT_MAX : (int)(total + 1);
}

__global__ __launch_bounds__(FL_THREADS) void flatten_count_kernel(FlattenParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * FL_WAVES + wave;
  if (s >= q.S) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.G, beg, n);
  if (n == 0) {
    if (lane == 0) q.counts[s] = 0;
    return;
  }
  const double* ctrl = q.ctrl + (size_t)beg * 8;
  const int* kind = q.kind + (size_t)beg;
  long long* E = q.E + (size_t)beg;
  long long carry = 0;
  for (long long k0 = 0; k0 < n; k0 += 64) {                                   // (the trip count is the same for every lane)
    const long long k = k0 + lane;
    long long v = 0;
    if (k < n) v = flatten_pieces(ctrl + k * 8, kind[k], q.c);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    if (k < n) E[k] = carry + v;
    carry += __shfl(v, 63, 64);
  }
  if (lane == 0) q.counts[s] = flatten_rows(carry);
}

__device__ __forceinline__ double flatten_lerp(double a, double b, double t) { return a + t * (b - a); }

// de Casteljau at t on one coordinate (stride 2 doubles from control point to control point): q0 q1 q2 r0 r1 s
__device__ __forceinline__ float flatten_eval(const double* p, double t) {
  const double p0 = p[0], p1 = p[2], p2 = p[4], p3 = p[6];
  const double q0 = flatten_lerp(p0, p1, t), q1 = flatten_lerp(p1, p2, t), q2 = flatten_lerp(p2, p3, t);
  const double r0 = flatten_lerp(q0, q1, t), r1 = flatten_lerp(q1, q2, t);
  return (float)flatten_lerp(r0, r1, t);
}

// Row m, 1 <= m <= E[n - 1], of the subpath with the control points ctrl, n >= 1 segments and the table E.
__device__ __forceinline__ float2 flatten_at(const double* ctrl, const long long* E, int n, long long m) {
  int lo = 0, hi = n - 1;                                                      // the smallest k with E[k] >= m
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (E[mid] >= m) hi = mid; else lo = mid + 1;
  }
  const long long prev = lo > 0 ? E[lo - 1] : 0;
  const long long pieces = E[lo] - prev, j = m - prev;                         // 1 <= j <= pieces
  const double* p = ctrl + (size_t)lo * 8;
  if (j >= pieces) return make_float2((float)p[6], (float)p[7]);               // the segment's end: copied, not evaluated
  const double t = (double)j / (double)pieces;
  return make_float2(flatten_eval(p, t), flatten_eval(p + 1, t));
}

__global__ __launch_bounds__(FL_THREADS) void flatten_emit_kernel(FlattenParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * FL_WAVES + wave;
  if (s >= q.S) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.G, beg, n);
  if (n == 0) return;
  const double* ctrl = q.ctrl + (size_t)beg * 8;
  const long long* E = q.E + (size_t)beg;
  const int rows = flatten_rows(E[n - 1]);
  const long long o = q.out_offsets[s];
  float2* out = (float2*)q.out_xy;
  // rows o + m, m = 0 .. rows - 1; only those inside [0, out_rows) are looked at
  for (long long m0 = o < 0 ? ((-o) & ~63ll) : 0; m0 < rows && o + m0 < q.out_rows; m0 += 64) {
    const long long m = m0 + lane, row = o + m;
    if (m >= rows || row < 0 || row >= q.out_rows) continue;
    if (m == 0) out[row] = make_float2((float)ctrl[0], (float)ctrl[1]);
    else out[row] = flatten_at(ctrl, E, n, m);
  }
}

size_t flatten_carve(void* ws, long long G, int S, FlattenParams& q) {
  SkfWsCarver c(ws);
  q.counts = c.take<int>(S); q.E = c.take<long long>(G);
  return c.used;
}

bool flatten_tol_ok(double tol) { return tol > 0.0 && tol < INFINITY; }         // (false for a NaN)

// c = (16 / 9) * tol^2: three fp64 roundings, the quotient first, then tol * tol, then their product
double flatten_c(double tol) {
  const double k = 16.0 / 9.0, t2 = tol * tol;
  return k * t2;
}

}  // namespace

extern "C" size_t skf_path_flatten_workspace_bytes(long long G, int S) {
  if (G < 1 || G >= (1ll << 31) || S < 1) return 0;
  FlattenParams q;
  return flatten_carve(nullptr, G, S, q);
}

#define FLATTEN_CHECK_ARGS()                                                                                                       \
  SKF_CHECK_ARG(ctrl && kind && path_offsets && workspace, "null pointer");                                                        \
  SKF_CHECK_ARG(S >= 1, "S must be at least 1");                                                                                   \
  SKF_CHECK_ARG(G >= 1 && G < (1ll << 31), "G must be in [1, 2^31)");                                                              \
  SKF_CHECK_ARG(((uintptr_t)ctrl & 7) == 0 && ((uintptr_t)kind & 3) == 0 && ((uintptr_t)path_offsets & 7) == 0 &&                  \
                    ((uintptr_t)workspace & 15) == 0,                                                                              \
                "ctrl, kind and path_offsets must be aligned to their element, the workspace to 16 bytes");                        \
  SKF_CHECK_ARG(workspace_bytes >= skf_path_flatten_workspace_bytes(G, S), "workspace too small");                                 \
  SKF_CHECK_ARG(flatten_tol_ok(tol), "tol must be finite and above 0")

extern "C" int skf_path_flatten_count(const double* ctrl, const int* kind, long long G, const long long* path_offsets, int S, double tol,
                                      long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  FLATTEN_CHECK_ARGS();
  SKF_CHECK_ARG(out_offsets && ((uintptr_t)out_offsets & 7) == 0, "out_offsets must be an 8-byte aligned pointer");
  hipStream_t st = (hipStream_t)stream;
  FlattenParams q = {};
  q.ctrl = ctrl; q.kind = kind; q.G = G; q.offsets = path_offsets; q.S = S; q.c = flatten_c(tol);
  flatten_carve(workspace, G, S, q);
  hipLaunchKernelGGL(flatten_count_kernel, dim3(skf_cdiv(S, FL_WAVES)), dim3(FL_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  skf_counts_to_offsets_launch(q.counts, S, out_offsets, st);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_path_flatten_emit(const double* ctrl, const int* kind, long long G, const long long* path_offsets, int S, double tol,
                                     const long long* out_offsets, float* out_xy, long long out_rows, void* workspace,
                                     size_t workspace_bytes, skf_stream_t stream) {
  FLATTEN_CHECK_ARGS();
  SKF_CHECK_ARG(out_offsets && out_xy && ((uintptr_t)out_offsets & 7) == 0 && ((uintptr_t)out_xy & 7) == 0,
                "out_offsets and out_xy must be 8-byte aligned pointers");
  SKF_CHECK_ARG(out_rows >= 1 && out_rows < (1ll << 31), "out_rows must be in [1, 2^31)");
  FlattenParams q = {};
  q.ctrl = ctrl; q.kind = kind; q.G = G; q.offsets = path_offsets; q.S = S; q.c = flatten_c(tol);
  q.out_offsets = out_offsets; q.out_xy = out_xy; q.out_rows = out_rows;
  flatten_carve(workspace, G, S, q);
  hipLaunchKernelGGL(flatten_emit_kernel, dim3(skf_cdiv(S, FL_WAVES)), dim3(FL_THREADS), 0, (hipStream_t)stream, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
