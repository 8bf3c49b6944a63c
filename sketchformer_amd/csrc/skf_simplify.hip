// Stroke simplification on the device (include/skf.h: skf_rdp_f32, skf_stroke3_simplify): Ramer-Douglas-Peucker by the rule the
// header states, bit-equal to the host restatement of tests/simplify_reference.py.  DESIGN.md section 3p.
//
// What decides correctness here:
//   * The rule has no division and no square root: a point is kept when m_k > eps^2 * L2, every operation rounded to fp64 on its
//     own.  This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS) and carries the pragma below as well.
//   * The kept set depends on per-segment decisions alone, so the recursion is run LEVEL BY LEVEL: every live segment of a level
//     is examined at once.  One wavefront owns one polyline (a stroke; for skf_stroke3_simplify a whole sketch, whose stroke ends
//     and stroke starts are kept from the beginning: neighbouring strokes are segments without an interior) and walks it in tiles
//     of 64 points:
//       pass A, backwards: every point learns the lowest kept index at or behind it (a ballot per tile, a carry between tiles);
//       pass B, forwards:  every undecided point of a live segment learns the highest kept index in front of it the same way,
//                          computes its m, and a segmented arg-max scan (shuffles, a carry between tiles; among equal m the lower
//                          index wins) leaves the segment's choice with its last interior point, which decides: keep k, or
//                          settle the segment (mark 2 on its left end: nothing between its ends is ever looked at again).
//     The loop ends with the level that keeps nothing.  A zigzag of shrinking amplitude needs n - 1 levels.
//   * Pass B writes marks while it walks, but only at indices of tiles it has already read, and the arg-max is taken over values,
//     not over arrival order: no atomics, and two calls agree bit for bit.
//   * The absolute positions of skf_stroke3_simplify are the sequential fp32 running sum of the grid tokenizer (one add per point):
//     one lane walks the sketch, the other lanes wait.
// A polyline of up to SKF_RDP_LDS_POINTS points lives in LDS (points, marks, the pass-A indices: 13 bytes a point); a longer one
// runs the same code on the workspace.  Lanes of a wave exchange data through memory between the passes: wave_fence().
#include "skf_ragged.h"
#include <float.h>
#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int RDP_WAVES = 4;              // polylines per workgroup, one wave each; 4 x 13 x 512 B = 26 KiB of LDS
constexpr int RDP_THREADS = 64 * RDP_WAVES;
constexpr int RDP_LDS = SKF_RDP_LDS_POINTS;

// What one lane wrote, every lane of the wave may read behind this.  Writer and readers are lanes of ONE wave, hence of one
// workgroup on one CU: a workgroup-scope fence orders the wave's earlier stores - to LDS and, in the workspace form, to global
// memory, where they go through the CU's own cache - before its later loads.  No other wave ever reads a polyline's marks or rgt
// inside a launch; the next launch sees them because a kernel's stores are visible at its end.
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The level loop over one polyline of n points: xy[i * ld], xy[i * ld + 1]; mark[i]: 0 undecided, 1 kept, 2 kept and the segment
// to its right settled; on entry the ends (and whatever else is kept from the start) carry 1 and everything else 0; rgt: n ints of
// scratch.  On exit mark[i] != 0 is the kept set.
__device__ __forceinline__ void rdp_levels(const float* xy, long long ld, unsigned char* mark, int* rgt, int n, double eps2, int lane) {
  if (n <= 2) return;
  const int tiles = (int)(((long long)n + 63) >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;                      // the lanes in front of this one
  for (;;) {
    // pass A: rgt[i] = the lowest kept index >= i (the last point is kept)
    int rcarry = INT_MAX;
    for (int t = tiles - 1; t >= 0; --t) {
      const long long i = (long long)t * 64 + lane;
      const unsigned long long kept = __ballot(i < n && mark[i] != 0);
      const unsigned long long here = kept & ~below;
      const int b = here ? t * 64 + __builtin_ctzll(here) : rcarry;
      if (i < n) rgt[i] = b;
      if (kept) rcarry = t * 64 + __builtin_ctzll(kept);
    }
    wave_fence();
    // pass B.  It decides by pass A's snapshot (rgt) although it writes marks as it goes, and stays consistent with it because,
    // within one tile iteration, the wave runs in lockstep with no fence in between: every lane's reads of mark[i] and mark[a]
    // come before any lane's writes of mark[k] and mark[a] further down.  Across iterations a write lands at k <= i or at the
    // left end a < i of a segment whose last interior point is in this tile: a later tile's lanes lie at or behind that segment's
    // right end b (kept in the snapshot already), so the left end they read is >= b, a kept index that no one writes before its
    // own segment has spoken.  Reordering the reads behind the writes, or splitting a tile between waves, would break this.
    int lcarry = -1, ck = 0;
    double cm = -1.0;
    bool any = false;
    for (int t = 0; t < tiles; ++t) {
      const long long i = (long long)t * 64 + lane;
      const int mk = i < n ? mark[i] : 1;
      const unsigned long long kept = __ballot(i < n && mk != 0);
      const unsigned long long upto = kept & (below | (1ull << lane));
      const int a = upto ? t * 64 + 63 - __builtin_clzll(upto) : lcarry;       // the highest kept index <= i (point 0 is kept)
      if (kept) lcarry = t * 64 + 63 - __builtin_clzll(kept);
      const bool live = mk == 0 && a >= 0 && mark[a] == 1;
      double m = -1.0, L2 = 1.0;
      int k = (int)i, b = 0;
      if (live) {
        b = rgt[i];
        const double xa = (double)xy[a * ld], ya = (double)xy[a * ld + 1];
        const double ex = (double)xy[b * ld] - xa, ey = (double)xy[b * ld + 1] - ya;
        const double px = (double)xy[i * ld] - xa, py = (double)xy[i * ld + 1] - ya;
        if (ex == 0.0 && ey == 0.0) {
          m = px * px + py * py;
        } else {
          const double c = ex * py - ey * px;
          m = c * c;
          L2 = ex * ex + ey * ey;
        }
      }
      // the interior of a live segment is a run of live lanes: lane - d belongs to this lane's segment iff it lies behind a
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double um = __shfl_up(m, d, 64);
        const int uk = __shfl_up(k, d, 64);
        if (live && lane >= d && i - d > a && um >= m) { m = um; k = uk; }   // (equal m: the lower index stays)
      }
      if (live && a < t * 64 - 1 && cm >= m) { m = cm; k = ck; }               // the part of the segment in the tiles before
      cm = __shfl(m, 63, 64);
      ck = __shfl(k, 63, 64);
      if (live && i + 1 == b) {                                                // the last interior point speaks for the segment
        if (m > eps2 * L2) { mark[k] = 1; any = true; }
        else mark[a] = 2;
      }
    }
    wave_fence();
    if (!__any(any)) break;
  }
}

struct RdpParams {
  const float* xy;              // (P, 2) absolute points, ldp floats from row to row
  long long ldp, P;
  const long long* offsets;     // S + 1
  int S;
  double eps2;
  unsigned char* keep;          // P
  unsigned char* mark;          // workspace, P: the marks of a polyline too long for LDS
  int* rgt;                     // workspace, P: its pass-A indices
};

__global__ __launch_bounds__(RDP_THREADS) void rdp_keep_kernel(RdpParams q) {
  __shared__ float s_xy[RDP_WAVES][2 * RDP_LDS];
  __shared__ int s_rgt[RDP_WAVES][RDP_LDS];
  __shared__ unsigned char s_mark[RDP_WAVES][RDP_LDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * RDP_WAVES + wave;
  if (s >= q.S) return;                                                        // (no workgroup barrier anywhere below)
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  if (n == 0) return;
  const float* src = q.xy + (size_t)beg * q.ldp;
  unsigned char* keep = q.keep + (size_t)beg;
  if (n <= RDP_LDS) {
    for (int i = lane; i < n; i += 64) {
      s_xy[wave][2 * i] = src[i * q.ldp];
      s_xy[wave][2 * i + 1] = src[i * q.ldp + 1];
      s_mark[wave][i] = (i == 0 || i == n - 1) ? 1 : 0;
    }
    wave_fence();
    rdp_levels(s_xy[wave], 2, s_mark[wave], s_rgt[wave], n, q.eps2, lane);
    for (int i = lane; i < n; i += 64) keep[i] = s_mark[wave][i] != 0 ? 1 : 0;
  } else {
    unsigned char* mark = q.mark + (size_t)beg;
    for (long long i = lane; i < n; i += 64) mark[i] = (i == 0 || i == n - 1) ? 1 : 0;
    wave_fence();
    rdp_levels(src, q.ldp, mark, q.rgt + (size_t)beg, n, q.eps2, lane);
    for (long long i = lane; i < n; i += 64) keep[i] = mark[i] != 0 ? 1 : 0;
  }
}

struct SimplifyParams {
  const float* flat;            // (P, 3) rows (dx, dy, pen)
  const long long* offsets;     // N + 1
  long long P;
  int N;
  double eps2;
  float* out_flat;              // (P, 3) capacity
  long long* out_offsets;       // N + 1
  int* counts;                  // workspace: kept rows per sketch
  unsigned char* mark;          // workspace, P: != 0 = kept
  float* pos;                   // workspace, (P, 2): absolute positions
  int* rgt;                     // workspace, P
};

// a row is kept from the start when it is the sketch's first or last, ends a stroke (pen == 1) or follows the end of one
__device__ __forceinline__ unsigned char simplify_seed(const float* rows, long long i, int n) {
  return (i == 0 || i == n - 1 || rows[3 * i + 2] == 1.0f || rows[3 * (i - 1) + 2] == 1.0f) ? 1 : 0;
}

// Launch 1.  Per sketch: absolute positions (sequential fp32 sums), the level loop over the whole sketch, the marks, the positions
// and the number of kept rows to the workspace.
__global__ __launch_bounds__(RDP_THREADS) void simplify_mark_kernel(SimplifyParams q) {
  __shared__ float s_xy[RDP_WAVES][2 * RDP_LDS];
  __shared__ int s_rgt[RDP_WAVES][RDP_LDS];
  __shared__ unsigned char s_mark[RDP_WAVES][RDP_LDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * RDP_WAVES + wave;
  if (s >= q.N) return;                                                        // (no workgroup barrier anywhere below)
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  if (n == 0) {
    if (lane == 0) q.counts[s] = 0;
    return;
  }
  const float* rows = q.flat + 3 * (size_t)beg;
  unsigned char* mark = q.mark + (size_t)beg;
  float* pos = q.pos + 2 * (size_t)beg;
  int kept = 0;
  if (n <= RDP_LDS) {
    float* xy = s_xy[wave];
    for (int i = lane; i < n; i += 64) {
      xy[2 * i] = rows[3 * i];
      xy[2 * i + 1] = rows[3 * i + 1];
      s_mark[wave][i] = simplify_seed(rows, i, n);
    }
    wave_fence();
    if (lane == 0) {
      float ax = 0.0f, ay = 0.0f;
      for (int i = 0; i < n; ++i) {
        ax = ax + xy[2 * i];
        ay = ay + xy[2 * i + 1];
        xy[2 * i] = ax;
        xy[2 * i + 1] = ay;
      }
    }
    wave_fence();
    rdp_levels(xy, 2, s_mark[wave], s_rgt[wave], n, q.eps2, lane);
    for (int i0 = 0; i0 < n; i0 += 64) {                                       // (the trip count is the same for every lane)
      const int i = i0 + lane;
      const unsigned char mk = i < n ? s_mark[wave][i] : 0;
      if (i < n) { mark[i] = mk; pos[2 * i] = xy[2 * i]; pos[2 * i + 1] = xy[2 * i + 1]; }
      kept += __popcll(__ballot(mk != 0));
    }
  } else {
    for (long long i = lane; i < n; i += 64) mark[i] = simplify_seed(rows, i, n);
    if (lane == 0) {
      float ax = 0.0f, ay = 0.0f;
      for (long long i = 0; i < n; ++i) {
        ax = ax + rows[3 * i];
        ay = ay + rows[3 * i + 1];
        pos[2 * i] = ax;
        pos[2 * i + 1] = ay;
      }
    }
    wave_fence();
    rdp_levels(pos, 2, mark, q.rgt + (size_t)beg, n, q.eps2, lane);
    for (long long i0 = 0; i0 < n; i0 += 64) {
      const long long i = i0 + lane;
      kept += __popcll(__ballot(i < n && mark[i] != 0));
    }
  }
  if (lane == 0) q.counts[s] = kept;
}

// Launch 2 is the shared counts -> offsets scan (skf_ragged.hip).

// Launch 3.  Per sketch: a kept row goes to out_offsets[s] + its rank among the kept rows, as (A - A_prev, pen): one fp32
// subtraction per coordinate, A_prev the position of the kept row before it in the sketch, (0, 0) for the first.
__global__ __launch_bounds__(RDP_THREADS) void simplify_write_kernel(SimplifyParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * RDP_WAVES + wave;
  if (s >= q.N) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  if (n == 0) return;
  const float* rows = q.flat + 3 * (size_t)beg;
  const unsigned char* mark = q.mark + (size_t)beg;
  const float* pos = q.pos + 2 * (size_t)beg;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long o = q.out_offsets[s];
  long long prev_carry = -1;
  for (long long i0 = 0; i0 < n; i0 += 64) {                                   // (the trip count is the same for every lane)
    const long long i = i0 + lane;
    const bool k = i < n && mark[i] != 0;
    const unsigned long long kept = __ballot(k);
    const unsigned long long front = kept & below;
    const long long prev = front ? i0 + 63 - __builtin_clzll(front) : prev_carry;
    const long long row = o + __popcll(front);
    // (row < P: offsets that overlap - the caller's error - would count more rows than out_flat holds)
    if (k && row < q.P) {
      const float px = prev >= 0 ? pos[2 * prev] : 0.0f, py = prev >= 0 ? pos[2 * prev + 1] : 0.0f;
      float* r = q.out_flat + 3 * (size_t)row;
      r[0] = pos[2 * i] - px;
      r[1] = pos[2 * i + 1] - py;
      r[2] = rows[3 * i + 2];
    }
    o += __popcll(kept);
    if (kept) prev_carry = i0 + 63 - __builtin_clzll(kept);
  }
}

// the workspaces of skf_rdp_f32 and skf_stroke3_simplify; each returns its size
size_t rdp_carve(void* ws, long long P, RdpParams& q) {
  SkfWsCarver c(ws);
  q.mark = c.take<unsigned char>(P); q.rgt = c.take<int>(P);
  return c.used;
}
size_t simplify_carve(void* ws, long long P, int N, SimplifyParams& q) {
  SkfWsCarver c(ws);
  q.counts = c.take<int>(N); q.mark = c.take<unsigned char>(P); q.pos = c.take<float>(2 * (size_t)P); q.rgt = c.take<int>(P);
  return c.used;
}

bool rdp_epsilon_ok(double e) { return e >= 0.0 && e <= DBL_MAX; }             // (false for a NaN)

}  // namespace

extern "C" size_t skf_rdp_workspace_bytes(long long P) {
  if (P < 1 || P >= (1ll << 31)) return 0;
  RdpParams q;
  return rdp_carve(nullptr, P, q);
}

extern "C" int skf_rdp_f32(const float* xy, int ldp, long long P, const long long* stroke_offsets, int S, double epsilon,
                           unsigned char* keep, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(xy, P, stroke_offsets, S, workspace, workspace_bytes, skf_rdp_workspace_bytes(P));
  SKF_CHECK_ARG(keep, "null pointer");
  SKF_CHECK_ARG(ldp >= 2, "ldp must be at least 2");
  SKF_CHECK_ARG(rdp_epsilon_ok(epsilon), "epsilon must be finite and not negative");
  RdpParams q;
  q.xy = xy; q.ldp = ldp; q.P = P; q.offsets = stroke_offsets; q.S = S; q.eps2 = epsilon * epsilon; q.keep = keep;
  rdp_carve(workspace, P, q);
  hipLaunchKernelGGL(rdp_keep_kernel, dim3(skf_cdiv(S, RDP_WAVES)), dim3(RDP_THREADS), 0, (hipStream_t)stream, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" size_t skf_stroke3_simplify_workspace_bytes(long long P, int N) {
  if (P < 1 || P >= (1ll << 31) || N < 1) return 0;
  SimplifyParams q;
  return simplify_carve(nullptr, P, N, q);
}

extern "C" int skf_stroke3_simplify(const float* flat, long long P, const long long* offsets, int N, double epsilon, unsigned flags,
                                    float* out_flat, long long* out_offsets, void* workspace, size_t workspace_bytes,
                                    skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(flat, P, offsets, N, workspace, workspace_bytes, skf_stroke3_simplify_workspace_bytes(P, N));
  SKF_CHECK_ARG(out_flat && out_offsets, "null pointer");
  SKF_CHECK_ARG(rdp_epsilon_ok(epsilon), "epsilon must be finite and not negative");
  SKF_CHECK_ARG(flags == 0, "unknown flag");
  SKF_CHECK_ARG(((uintptr_t)out_flat & 3) == 0 && ((uintptr_t)out_offsets & 7) == 0, "out_flat, out_offsets must be aligned to their element");
  hipStream_t st = (hipStream_t)stream;
  SimplifyParams q;
  q.flat = flat; q.offsets = offsets; q.P = P; q.N = N; q.eps2 = epsilon * epsilon; q.out_flat = out_flat; q.out_offsets = out_offsets;
  simplify_carve(workspace, P, N, q);

  hipLaunchKernelGGL(simplify_mark_kernel, dim3(skf_cdiv(N, RDP_WAVES)), dim3(RDP_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  skf_counts_to_offsets_launch(q.counts, N, out_offsets, st);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(simplify_write_kernel, dim3(skf_cdiv(N, RDP_WAVES)), dim3(RDP_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
