// Stroke edits on the device (include/skf.h: skf_stroke_table, skf_stroke_edit_count / _emit): new sketches built out of the strokes
// of old ones, in any order, forwards or backwards, some left out, the pen jumps between them recomputed; bit-equal to the host
// restatement of tests/strokes_reference.py.  DESIGN.md section 3u.
//
// What decides correctness here:
//   * The only rounded operations are the absolute positions (the sequential fp32 running sum of skf_stroke3_simplify: one lane
//     walks the sketch, the other lanes wait) and one fp32 subtraction per coordinate for the first row of every selected stroke.
//     Everything else is a copy or a sign flip of stored bits.  This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS)
//     and carries the pragma below as well, although no product stands next to a sum here.
//   * Table, launch 1: one wavefront per sketch counts its stroke ends (pen == 1, or the sketch's last row) with a ballot per tile
//     of 64 rows.  The shared counts -> offsets scan (skf_ragged.hip) gives sketch_strokes.  Launch 2: one wavefront per sketch again;
//     the positions of a sketch of up to ST_LDS rows live in LDS, those of a longer one in the workspace; a stroke end's rank within
//     the sketch is the popcount of the ends below its lane plus the carry of the tiles before, its first row the row behind the end
//     before it.
//   * Edit, count launch: one wavefront per output sketch walks its selection list in tiles of 64 entries: the entry's stroke (or
//     -1: absent), its length, and through a wave scan with a carry its first row inside the output sketch; the sketch's row count.
//     The shared scan gives out_offsets.  Emit launch: a wavefront takes 64 entries at a time.  Every lane gathers what one entry
//     needs (its source rows, its first output row, its first output row's VALUE: where the stroke is entered less where the pen
//     comes from, read from stroke_ends of the present entry in front, walking back over absent ones); then every lane takes one
//     output ROW of the tile at a time, consecutive lanes consecutive rows (64 rows = one contiguous run of 768 bytes), and finds
//     the entry that owns it by binary search over the tile's 64 starts in LDS.  Of the three layouts measured this one is 4 to 5
//     times faster than a wave per entry and than a lane per row searching through memory (profiles/stroke_edit_bench.txt).
//   * Every range read from offsets, sketch_strokes, stroke_rows, src, sel_offsets or sel is clamped before it is an index, every
//     store to the capacity the caller states.
// No atomics, no allocation, no host synchronisation; every output element has one writer.
#include "skf_ragged.h"
#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int ST_WAVES = 4;               // sketches (table, count) or tiles of 64 entries (emit) per workgroup, one wave each
constexpr int ST_THREADS = 64 * ST_WAVES;
constexpr int ST_LDS = 512;               // rows of a sketch whose positions stay on chip: 4 x 512 x 8 B = 16 KiB of LDS
constexpr int ST_EMIT_BLOCKS = 2048;      // the emit grid: 8 workgroups on each of 256 CUs, all resident at once

// what one lane wrote, every lane of the same wave may read behind this (skf_simplify.hip has the reasoning)
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct TableParams {
  const float* flat;            // (P, 3) rows (dx, dy, pen)
  const long long* offsets;     // N + 1
  long long P;
  int N;
  long long* sketch_strokes;    // N + 1
  long long* stroke_rows;       // P + 1 capacity
  float* stroke_ends;           // (P, 4) capacity
  int* counts;                  // workspace, N: strokes per sketch
  float* pos;                   // workspace, (P, 2): the positions of a sketch too long for LDS
};

// row i of a sketch of n rows ends a stroke
__device__ __forceinline__ bool stroke_end(const float* rows, long long i, int n) { return rows[3 * i + 2] == 1.0f || i == n - 1; }

__global__ __launch_bounds__(ST_THREADS) void stroke_count_kernel(TableParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * ST_WAVES + wave;
  if (s >= q.N) return;
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  const float* rows = q.flat + 3 * (size_t)beg;
  int strokes = 0;
  for (long long i0 = 0; i0 < n; i0 += 64) {                                   // (the trip count is the same for every lane)
    const long long i = i0 + lane;
    strokes += __popcll(__ballot(i < n && stroke_end(rows, i, n)));
  }
  if (lane == 0) q.counts[s] = strokes;
}

__global__ __launch_bounds__(ST_THREADS) void stroke_write_kernel(TableParams q) {
  __shared__ float s_pos[ST_WAVES][2 * ST_LDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * ST_WAVES + wave;
  if (s >= q.N) return;                                                        // (no workgroup barrier anywhere below)
  long long beg;
  int n;
  skf_ragged_range(q.offsets, s, q.P, beg, n);
  // the entry behind the last stroke: the end of the rows.  (T > P needs offsets that overlap, the caller's error: the table is
  // then cut at its capacity.)
  if (s == q.N - 1 && lane == 0) q.stroke_rows[clampll(q.sketch_strokes[q.N], 0, q.P)] = beg + n;
  if (n == 0) return;
  const float* rows = q.flat + 3 * (size_t)beg;
  float* pos;
  if (n <= ST_LDS) {
    pos = s_pos[wave];
    for (int i = lane; i < n; i += 64) {
      pos[2 * i] = rows[3 * i];
      pos[2 * i + 1] = rows[3 * i + 1];
    }
    wave_fence();
    if (lane == 0) {
      float ax = 0.0f, ay = 0.0f;
      for (int i = 0; i < n; ++i) {
        ax = ax + pos[2 * i];
        ay = ay + pos[2 * i + 1];
        pos[2 * i] = ax;
        pos[2 * i + 1] = ay;
      }
    }
  } else {
    pos = q.pos + 2 * (size_t)beg;
    if (lane == 0) {
      float ax = 0.0f, ay = 0.0f;
      for (long long i = 0; i < n; ++i) {
        ax = ax + rows[3 * i];
        ay = ay + rows[3 * i + 1];
        pos[2 * i] = ax;
        pos[2 * i + 1] = ay;
      }
    }
  }
  wave_fence();
  const unsigned long long below = (1ull << lane) - 1ull;                      // the lanes in front of this one
  long long g = q.sketch_strokes[s];                                           // the global index of the tile's first stroke
  long long prev_carry = -1;                                                   // the last stroke end of the tiles before
  for (long long i0 = 0; i0 < n; i0 += 64) {                                   // (the trip count is the same for every lane)
    const long long i = i0 + lane;
    const bool e = i < n && stroke_end(rows, i, n);
    const unsigned long long ends = __ballot(e);
    const unsigned long long front = ends & below;
    const long long first = (front ? i0 + 63 - __builtin_clzll(front) : prev_carry) + 1;
    const long long t = g + __popcll(front);
    if (e && t >= 0 && t < q.P) {
      q.stroke_rows[t] = beg + first;
      float* o = q.stroke_ends + 4 * (size_t)t;
      o[0] = pos[2 * first];
      o[1] = pos[2 * first + 1];
      o[2] = pos[2 * i];
      o[3] = pos[2 * i + 1];
    }
    g += __popcll(ends);
    if (ends) prev_carry = i0 + 63 - __builtin_clzll(ends);
  }
}

struct EditParams {
  const float* flat;            // (P, 3)
  long long P;
  const long long* sketch_strokes;   // N + 1
  int N;
  const long long* stroke_rows; // T + 1
  const float* stroke_ends;     // (T, 4)
  long long T;
  const int* src;               // M
  const long long* sel_offsets; // M + 1
  int M;
  const int* sel;               // Q
  long long Q;
  const long long* out_offsets; // M + 1: what the scan wrote
  float* out_flat;              // (out_rows, 3)
  long long out_rows;
  int* counts;                  // workspace, M: rows per output sketch
  int* ent_stroke;              // workspace, Q: the global stroke of an entry, -1 = absent
  int* ent_owner;               // workspace, Q: the output sketch of an entry, -1 = in no list
  long long* ent_first;         // workspace, Q: the entry's first row inside its output sketch
};

// the entries [q0, q1) that output sketch m lists
__device__ __forceinline__ void edit_list(const EditParams& q, long long m, long long& q0, long long& q1) {
  q0 = clampll(q.sel_offsets[m], 0, q.Q);
  q1 = clampll(q.sel_offsets[m + 1], q0, q.Q);
}

// the rows [a, a + len) of stroke g, 0 <= g < T
__device__ __forceinline__ void edit_stroke_rows(const EditParams& q, long long g, long long& a, long long& len) {
  a = clampll(q.stroke_rows[g], 0, q.P);
  len = clampll(q.stroke_rows[g + 1], a, q.P) - a;
}

__global__ __launch_bounds__(ST_THREADS) void edit_count_kernel(EditParams q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * ST_WAVES + wave;
  if (m >= q.M) return;
  const int s = q.src[m];
  long long g0 = 0, ns = 0;                                                    // the source's strokes g0 .. g0 + ns - 1
  if (s >= 0 && s < q.N) {
    g0 = clampll(q.sketch_strokes[s], 0, q.T);
    ns = clampll(q.sketch_strokes[s + 1], g0, q.T) - g0;
  }
  long long q0, q1;
  edit_list(q, m, q0, q1);
  long long carry = 0;
  for (long long e0 = q0; e0 < q1; e0 += 64) {                                 // (the trip count is the same for every lane)
    const long long e = e0 + lane;
    long long g = -1, len = 0;
    if (e < q1) {
      const int k = q.sel[e];
      const long long kk = k < 0 ? ~k : k;
      if (kk < ns) {
        long long a;
        g = g0 + kk;
        edit_stroke_rows(q, g, a, len);
        if (len == 0) g = -1;                                                  // (a table that says so: absent like any other)
      }
    }
    long long v = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    if (e < q1) {
      q.ent_stroke[e] = (int)g;                                                // T <= P < 2^31
      q.ent_owner[e] = (int)m;
      q.ent_first[e] = carry + v - len;
    }
    carry += __shfl(v, 63, 64);
  }
  if (lane == 0) q.counts[m] = carry >= (long long)INT_MAX ? INT_MAX : (int)carry;
}

// What emit needs to know about one entry: one lane gathers it, every lane of the wave reads it from LDS.
struct EmitEntry {
  long long first;              // its first row of out_flat
  long long a;                  // its first source row
  long long len;                // its rows, 0 = absent
  float fx, fy;                 // its first output row: where the stroke is entered less where the pen comes from
  int back;
};

__device__ __forceinline__ EmitEntry edit_emit_header(const EditParams& q, long long e) {
  EmitEntry h = {0, 0, 0, 0.0f, 0.0f, 0};
  if (e >= q.Q) return h;
  const long long m = q.ent_owner[e], g = q.ent_stroke[e];
  if (m < 0 || m >= q.M || g < 0 || g >= q.T) return h;
  long long q0, q1;
  edit_list(q, m, q0, q1);
  if (e < q0 || e >= q1) return h;
  long long a, len;
  edit_stroke_rows(q, g, a, len);
  h.first = q.out_offsets[m] + q.ent_first[e];
  if (h.first >= q.out_rows || h.first + len <= 0) return h;
  h.a = a;
  h.len = len;
  h.back = q.sel[e] < 0;
  // where the pen comes from: the end of the present entry in front
  float ex = 0.0f, ey = 0.0f;
  for (long long j = e - 1; j >= q0; --j) {
    const long long gp = q.ent_stroke[j];
    if (gp < 0 || gp >= q.T) continue;
    const float* pe = q.stroke_ends + 4 * (size_t)gp + (q.sel[j] < 0 ? 0 : 2);
    ex = pe[0];
    ey = pe[1];
    break;
  }
  const float* ends = q.stroke_ends + 4 * (size_t)g + (h.back ? 2 : 0);        // the position of the first row drawn
  h.fx = ends[0] - ex;
  h.fy = ends[1] - ey;
  return h;
}

// A fixed grid of waves strides over the entries in tiles of 64.  A stroke is tens of rows: a wave that took one entry at a time
// waited four dependent loads long for every one of them.  Here every lane gathers the header of one entry of the tile, all 64
// chains in flight at once; a wave scan gives every entry its first row within the tile; then every lane takes one ROW of the tile
// at a time, consecutive lanes consecutive rows, and finds the entry that owns it by binary search over the 64 starts in LDS.
__global__ __launch_bounds__(ST_THREADS) void edit_emit_kernel(EditParams q) {
  __shared__ EmitEntry s_ent[ST_WAVES][64];
  __shared__ long long s_start[ST_WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  EmitEntry* ent = s_ent[wave];
  long long* start = s_start[wave];
  const long long stride = (long long)gridDim.x * ST_WAVES * 64;
  for (long long e0 = ((long long)blockIdx.x * ST_WAVES + wave) * 64; e0 < q.Q; e0 += stride) {    // (uniform within the wave)
    const EmitEntry h = edit_emit_header(q, e0 + lane);
    long long v = h.len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    const long long total = __shfl(v, 63, 64);
    ent[lane] = h;
    start[lane] = v - h.len;
    wave_fence();
    for (long long j = lane; j < total; j += 64) {
      int lo = 0, hi = 64;                                                     // the last entry with start <= j: an absent one
      while (hi - lo > 1) {                                                    // shares its start with the entry behind it
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= j) lo = mid; else hi = mid;
      }
      const EmitEntry k = ent[lo];
      const long long r = j - start[lo], row = k.first + r;
      if (r >= k.len || row < 0 || row >= q.out_rows) continue;
      float dx = k.fx, dy = k.fy;
      if (r > 0) {
        const float* in = q.flat + 3 * (size_t)(k.back ? k.a + k.len - r : k.a + r);
        dx = k.back ? -in[0] : in[0];
        dy = k.back ? -in[1] : in[1];
      }
      float* o = q.out_flat + 3 * (size_t)row;
      o[0] = dx;
      o[1] = dy;
      o[2] = r == k.len - 1 ? 1.0f : 0.0f;
    }
    wave_fence();                                                              // the next tile rewrites ent and start
  }
}

size_t table_carve(void* ws, long long P, int N, TableParams& q) {
  SkfWsCarver c(ws);
  q.counts = c.take<int>(N); q.pos = c.take<float>(2 * (size_t)P);
  return c.used;
}

size_t edit_carve(void* ws, int M, long long Q, EditParams& q) {
  SkfWsCarver c(ws);
  q.counts = c.take<int>(M); q.ent_stroke = c.take<int>(Q); q.ent_owner = c.take<int>(Q); q.ent_first = c.take<long long>(Q);
  return c.used;
}

bool edit_sizes_ok(long long P, int N, long long T, int M, long long Q) {
  return P >= 1 && P < (1ll << 31) && N >= 1 && M >= 1 && Q >= 0 && Q < (1ll << 31) && T >= 0 && T <= P;
}

}  // namespace

extern "C" size_t skf_stroke_table_workspace_bytes(long long P, int N) {
  if (P < 1 || P >= (1ll << 31) || N < 1) return 0;
  TableParams q;
  return table_carve(nullptr, P, N, q);
}

extern "C" int skf_stroke_table(const float* flat, long long P, const long long* offsets, int N, unsigned flags, long long* sketch_strokes,
                                long long* stroke_rows, float* stroke_ends, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(flat, P, offsets, N, workspace, workspace_bytes, skf_stroke_table_workspace_bytes(P, N));
  SKF_CHECK_ARG(sketch_strokes && stroke_rows && stroke_ends, "null pointer");
  SKF_CHECK_ARG(flags == 0, "unknown flag");
  SKF_CHECK_ARG(((uintptr_t)sketch_strokes & 7) == 0 && ((uintptr_t)stroke_rows & 7) == 0 && ((uintptr_t)stroke_ends & 3) == 0,
                "sketch_strokes, stroke_rows, stroke_ends must be aligned to their element");
  hipStream_t st = (hipStream_t)stream;
  TableParams q;
  q.flat = flat; q.offsets = offsets; q.P = P; q.N = N; q.sketch_strokes = sketch_strokes; q.stroke_rows = stroke_rows;
  q.stroke_ends = stroke_ends;
  table_carve(workspace, P, N, q);
  hipLaunchKernelGGL(stroke_count_kernel, dim3(skf_cdiv(N, ST_WAVES)), dim3(ST_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  skf_counts_to_offsets_launch(q.counts, N, sketch_strokes, st);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(stroke_write_kernel, dim3(skf_cdiv(N, ST_WAVES)), dim3(ST_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" size_t skf_stroke_edit_workspace_bytes(long long P, int N, int M, long long Q) {
  if (!edit_sizes_ok(P, N, 0, M, Q)) return 0;
  EditParams q;
  return edit_carve(nullptr, M, Q, q);
}

// the argument checks the two phases share
#define SKF_STROKE_EDIT_CHECK_ARGS()                                                                                             \
  SKF_CHECK_ARG(sketch_strokes && stroke_rows && src && sel_offsets && workspace, "null pointer");                               \
  SKF_CHECK_ARG(N >= 1 && M >= 1, "N and M must be at least 1");                                                                 \
  SKF_CHECK_ARG(P >= 1 && P < (1ll << 31), "P must be in [1, 2^31)");                                                            \
  SKF_CHECK_ARG(Q >= 0 && Q < (1ll << 31), "Q must be in [0, 2^31)");                                                            \
  SKF_CHECK_ARG(T >= 0 && T <= P, "T must be in [0, P]");                                                                        \
  SKF_CHECK_ARG(sel || Q == 0, "null pointer");                                                                                  \
  SKF_CHECK_ARG(flags == 0, "unknown flag");                                                                                     \
  SKF_CHECK_ARG(((uintptr_t)sketch_strokes & 7) == 0 && ((uintptr_t)stroke_rows & 7) == 0 && ((uintptr_t)sel_offsets & 7) == 0 && \
                ((uintptr_t)src & 3) == 0 && ((uintptr_t)sel & 3) == 0 && ((uintptr_t)workspace & 15) == 0,                      \
                "pointers must be aligned to their element, the workspace to 16 bytes");                                         \
  SKF_CHECK_ARG(workspace_bytes >= skf_stroke_edit_workspace_bytes(P, N, M, Q), "workspace too small")

extern "C" int skf_stroke_edit_count(long long P, const long long* sketch_strokes, int N, const long long* stroke_rows, long long T,
                                     const int* src, const long long* sel_offsets, int M, const int* sel, long long Q, unsigned flags,
                                     long long* out_offsets, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_STROKE_EDIT_CHECK_ARGS();
  SKF_CHECK_ARG(out_offsets && ((uintptr_t)out_offsets & 7) == 0, "out_offsets must be an 8-byte aligned pointer");
  hipStream_t st = (hipStream_t)stream;
  EditParams q = {};
  q.P = P; q.sketch_strokes = sketch_strokes; q.N = N; q.stroke_rows = stroke_rows; q.T = T; q.src = src; q.sel_offsets = sel_offsets;
  q.M = M; q.sel = sel; q.Q = Q;
  edit_carve(workspace, M, Q, q);
  if (Q > 0) SKF_HIP(hipMemsetAsync(q.ent_owner, 0xff, (size_t)Q * sizeof(int), st));   // an entry outside every list has no owner
  hipLaunchKernelGGL(edit_count_kernel, dim3(skf_cdiv(M, ST_WAVES)), dim3(ST_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  skf_counts_to_offsets_launch(q.counts, M, out_offsets, st);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_stroke_edit_emit(const float* flat, long long P, const long long* sketch_strokes, int N, const long long* stroke_rows,
                                    const float* stroke_ends, long long T, const int* src, const long long* sel_offsets, int M,
                                    const int* sel, long long Q, unsigned flags, const long long* out_offsets, float* out_flat,
                                    long long out_rows, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_STROKE_EDIT_CHECK_ARGS();
  SKF_CHECK_ARG(flat && out_offsets && out_flat && (stroke_ends || T == 0), "null pointer");
  SKF_CHECK_ARG(((uintptr_t)flat & 3) == 0 && ((uintptr_t)stroke_ends & 3) == 0 && ((uintptr_t)out_offsets & 7) == 0 &&
                ((uintptr_t)out_flat & 3) == 0, "flat, stroke_ends, out_offsets, out_flat must be aligned to their element");
  SKF_CHECK_ARG(out_rows >= 1 && out_rows < (1ll << 31), "out_rows must be in [1, 2^31)");
  EditParams q = {};
  q.flat = flat; q.P = P; q.sketch_strokes = sketch_strokes; q.N = N; q.stroke_rows = stroke_rows; q.stroke_ends = stroke_ends; q.T = T;
  q.src = src; q.sel_offsets = sel_offsets; q.M = M; q.sel = sel; q.Q = Q; q.out_offsets = out_offsets; q.out_flat = out_flat;
  q.out_rows = out_rows;
  edit_carve(workspace, M, Q, q);
  if (Q == 0 || T == 0) return SKF_OK;                                         // nothing is listed, or nothing can be present
  const int blocks = skf_cdiv(Q, 64 * ST_WAVES);
  hipLaunchKernelGGL(edit_emit_kernel, dim3(blocks < ST_EMIT_BLOCKS ? blocks : ST_EMIT_BLOCKS), dim3(ST_THREADS), 0, (hipStream_t)stream, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
