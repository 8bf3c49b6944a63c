// Raw stroke-3 sketches -> model input on the device (include/skf.h: skf_nearest_center_f64, skf_sketch_encode): the loader's
// per-sketch pipeline (dataloaders/distributed_stroke3.py: preprocess_per_sketch_from; utils/tokenizer.py: Tokenizer.encode with
// its float64 nearest_center, GridTokenizer.encode) with the same operations in the same order and precision, so that the
// results are bit-equal to the host's.  DESIGN.md section 3m.
//
// Two things decide correctness here:
//   * Summation order is part of the definition.  The bounds are a float64 running sum and the grid positions an fp32 running sum,
//     one add per point in sequence; a tree or shuffle scan rounds differently and moves points across cell borders.  So the scans
//     are sequential: one LANE owns one sketch (a chunk holds tens of thousands of sketches, which is the parallelism), and the
//     work that is independent per point - the nearest centre, the scatter into the rows - runs point-parallel in launches of its
//     own.
//   * No contraction and no approximate division.  This file is compiled with -ffp-contract=off (build.SOURCE_FLAGS) and carries
//     the pragma below as well: every subtract, multiply and add is rounded on its own, and `/` is the correctly rounded fp32
//     division (the v_div_scale / v_div_fmas / v_div_fixup sequence).
//
// Launches of skf_sketch_encode: fill (rows := PAD, or the stroke-5 end row) -> scan (per sketch: bounds, divisor, normalised
// offsets, grid ids, every point's place in its row, SOS / EOS) -> [DICT: nearest centre] -> pack (per point: one or two stores).
// No atomics; every output element has one writer per launch and the launches are ordered by the stream.
#include "skf_ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int TOK_MAXK = 4096;
constexpr int NC_THREADS = 256;
constexpr int NC_PTS = 4;                 // points per thread: one LDS read of a centre serves four distances
constexpr int SCAN_THREADS = 64;          // one wave per workgroup: 70k sketches are ~1100 waves, spread over every CU
constexpr int PACK_THREADS = 256;

// ---------------------------------------------------------------- nearest centre, float64
// d = (x - cx)^2 + (y - cy)^2 with x, y widened to fp64 and each of the five operations rounded on its own; the lowest index wins
// among equal minima (strict < while walking k upwards).  Centres sit in LDS as (cx, cy) pairs: every lane reads the same address
// (a broadcast, no bank conflict), one ds_read_b128 per centre and four points.
__global__ __launch_bounds__(NC_THREADS) void nearest_center_kernel(const float* __restrict__ points, int ldp, long long P,
                                                                     const double* __restrict__ centers, int K,
                                                                     int* __restrict__ labels) {
  extern __shared__ double2 sC[];
  for (int k = threadIdx.x; k < K; k += NC_THREADS) sC[k] = make_double2(centers[2 * (size_t)k], centers[2 * (size_t)k + 1]);
  __syncthreads();
  const long long base = (long long)blockIdx.x * (NC_THREADS * NC_PTS) + threadIdx.x;
  double x[NC_PTS], y[NC_PTS], best[NC_PTS];
  int arg[NC_PTS];
#pragma unroll
  for (int j = 0; j < NC_PTS; ++j) {
    const long long p = base + (long long)j * NC_THREADS;
    const bool in = p < P;
    x[j] = in ? (double)points[(size_t)p * ldp] : 0.0;
    y[j] = in ? (double)points[(size_t)p * ldp + 1] : 0.0;
    const double dx = x[j] - sC[0].x, dy = y[j] - sC[0].y;
    best[j] = dx * dx + dy * dy;
    arg[j] = 0;
  }
  for (int k = 1; k < K; ++k) {
    const double2 c = sC[k];
#pragma unroll
    for (int j = 0; j < NC_PTS; ++j) {
      const double dx = x[j] - c.x, dy = y[j] - c.y;
      const double d = dx * dx + dy * dy;
      if (d < best[j]) { best[j] = d; arg[j] = k; }
    }
  }
#pragma unroll
  for (int j = 0; j < NC_PTS; ++j) {
    const long long p = base + (long long)j * NC_THREADS;
    if (p < P) labels[p] = arg[j];
  }
}

// ---------------------------------------------------------------- encode
struct EncodeParams {
  const float* flat;            // (P, 3) rows (dx, dy, pen)
  const long long* offsets;     // N + 1
  long long P;
  int N, mode, K, L, clamp;
  void* out;                    // (N, L) int64 or (N, L, 5) fp32
  float* scale;                 // N or null
  float2* xy;                   // workspace: normalised offsets per point (DICT, STROKE5)
  long long* ids;               // workspace: grid ids per point (GRID); the nearest-centre labels as int32 (DICT)
  long long* dst;               // workspace: per point, -1 = not stored, else 2 * (element index of its token / row) + (SEP follows)
};

__global__ __launch_bounds__(PACK_THREADS) void encode_fill_kernel(void* out, long long n, int stroke5) {
  const long long stride = (long long)gridDim.x * PACK_THREADS;
  for (long long i = (long long)blockIdx.x * PACK_THREADS + threadIdx.x; i < n; i += stride) {
    if (stroke5) ((float*)out)[i] = (i % 5 == 4) ? 1.0f : 0.0f;       // rows behind a sketch: (0, 0, 0, 0, 1)
    else ((long long*)out)[i] = 0;                                    // PAD
  }
}

// One lane per sketch.  Pass 1: the float64 running sums of the offsets, their extent with the origin included, the last pen
// lift and the number of lifts.  Pass 2: X = x / div, Y = y / div, the fp32 running sum and the cell of the grid path, and where
// the point goes in its row.
__global__ __launch_bounds__(SCAN_THREADS) void encode_scan_kernel(EncodeParams q) {
  const long long s = (long long)blockIdx.x * SCAN_THREADS + threadIdx.x;
  if (s >= q.N) return;
  long long beg_;
  int n_;
  skf_ragged_range(q.offsets, s, q.P, beg_, n_);
  const long long beg = beg_;                // (const copies: with the reference arguments themselves as the loop bounds below,
  const int n = n_;                          //  the compiler numbers this kernel's registers differently)
  const float* rows = q.flat + 3 * (size_t)beg;

  double cx = 0.0, cy = 0.0, min_x = 0.0, max_x = 0.0, min_y = 0.0, max_y = 0.0;
  int last = -1, nlift = 0;
  for (int t = 0; t < n; ++t) {
    cx = cx + (double)skf_sketch_clamp(rows[3 * t], q.clamp);
    cy = cy + (double)skf_sketch_clamp(rows[3 * t + 1], q.clamp);
    min_x = fmin(min_x, cx); max_x = fmax(max_x, cx);
    min_y = fmin(min_y, cy); max_y = fmax(max_y, cy);
    if (skf_sketch_clamp(rows[3 * t + 2], q.clamp) == 1.0f) { last = t; ++nlift; }
  }
  const float div = (float)fmax(fmax(max_x - min_x, max_y - min_y), 1.0);
  if (q.scale) q.scale[s] = div;
  if (n == 0) return;                                                        // the row stays all PAD / all end

  const int L = q.L;
  if (q.mode == SKF_ENCODE_STROKE5) {
    for (int t = 0; t < n; ++t) {
      const long long p = beg + t;
      q.xy[p] = make_float2(skf_sketch_clamp(rows[3 * t], q.clamp) / div, skf_sketch_clamp(rows[3 * t + 1], q.clamp) / div);
      q.dst[p] = t < L ? 2 * (s * L + t) : -1;
    }
    return;
  }
  const bool grid = q.mode == SKF_ENCODE_GRID;
  const long long R = q.K, vocab = grid ? R * R : (long long)q.K;           // SEP = vocab + 1, SOS = vocab + 2, EOS = vocab + 3
  long long* row = (long long*)q.out + (size_t)s * L;
  // grid: points behind the last lift are dropped; without a lift every point stays and one SEP closes the sketch
  const int stop = grid ? (nlift > 0 ? last + 1 : n) : n;
  const float half = (float)(R / 2);
  float gx = 0.0f, gy = 0.0f;
  long long pos = 1;
  for (int t = 0; t < n; ++t) {
    const long long p = beg + t;
    const float X = skf_sketch_clamp(rows[3 * t], q.clamp) / div, Y = skf_sketch_clamp(rows[3 * t + 1], q.clamp) / div;
    if (grid) {
      gx = gx + X; gy = gy + Y;
      long long ix = (long long)((gx + 1.0f) * half), iy = (long long)((gy + 1.0f) * half);
      if (ix == R) ix = R - 1;
      if (iy == R) iy = R - 1;
      q.ids[p] = ix + iy * R + 1;
    } else {
      q.xy[p] = make_float2(X, Y);
    }
    if (t >= stop) { q.dst[p] = -1; continue; }
    const bool sep = grid && nlift == 0 ? t == n - 1 : skf_sketch_clamp(rows[3 * t + 2], q.clamp) == 1.0f;
    q.dst[p] = pos < L ? 2 * (s * L + pos) + (sep && pos + 1 < L ? 1 : 0) : -1;
    pos += sep ? 2 : 1;
  }
  row[0] = vocab + 2;
  if (pos < L) row[pos] = vocab + 3;
}

__global__ __launch_bounds__(PACK_THREADS) void encode_pack_kernel(EncodeParams q) {
  const long long p = (long long)blockIdx.x * PACK_THREADS + threadIdx.x;
  if (p >= q.P) return;
  const long long d = q.dst[p];
  const long long e = d >> 1;
  // (a point that no sketch owns - offsets that do not cover flat - has no entry: whatever the workspace held stays in bounds)
  if (d < 0 || e + (d & 1) >= (long long)q.N * q.L) return;
  if (q.mode == SKF_ENCODE_STROKE5) {
    const float2 v = q.xy[p];
    const float pen = skf_sketch_clamp(q.flat[3 * (size_t)p + 2], q.clamp);
    float* r = (float*)q.out + 5 * (size_t)e;
    r[0] = v.x; r[1] = v.y; r[2] = 1.0f - pen; r[3] = pen;
    r[4] = (e % q.L == q.L - 1) ? 1.0f : 0.0f;                               // the last row always carries the end flag
    return;
  }
  long long* o = (long long*)q.out + e;
  o[0] = q.mode == SKF_ENCODE_GRID ? q.ids[p] : (long long)((const int*)q.ids)[p] + 1;
  if (d & 1) o[1] = (q.mode == SKF_ENCODE_GRID ? (long long)q.K * q.K : (long long)q.K) + 1;
}

// the workspace of skf_sketch_encode; returns its size
size_t encode_carve(void* ws, long long P, EncodeParams& q) {
  SkfWsCarver c(ws);
  q.xy = c.take<float2>(P); q.ids = c.take<long long>(P); q.dst = c.take<long long>(P);
  return c.used;
}

int nearest_center_launch(const float* points, int ldp, long long P, const double* centers, int K, int* labels, hipStream_t st) {
  const long long blocks = (P + NC_THREADS * NC_PTS - 1) / (NC_THREADS * NC_PTS);
  hipLaunchKernelGGL(nearest_center_kernel, dim3((unsigned)blocks), dim3(NC_THREADS), (size_t)K * sizeof(double2), st, points, ldp, P,
                     centers, K, labels);
  return SKF_OK;
}

}  // namespace

extern "C" int skf_nearest_center_f64(const float* points, int ldp, long long P, const double* centers, int K, int* labels,
                                      skf_stream_t stream) {
  SKF_CHECK_ARG(points && centers && labels, "null pointer");
  SKF_CHECK_ARG(P >= 1 && P < (1ll << 31), "P must be in [1, 2^31)");
  SKF_CHECK_ARG(K >= 1 && K <= TOK_MAXK, "K must be in [1, 4096]");
  SKF_CHECK_ARG(ldp >= 2, "ldp must be at least 2");
  SKF_CHECK_ARG(((uintptr_t)points & 3) == 0 && ((uintptr_t)centers & 7) == 0 && ((uintptr_t)labels & 3) == 0,
                "points, centers and labels must be aligned to their element");
  nearest_center_launch(points, ldp, P, centers, K, labels, (hipStream_t)stream);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" size_t skf_sketch_encode_workspace_bytes(long long P, int N) {
  if (P < 1 || P >= (1ll << 31) || N < 1) return 0;
  EncodeParams q;
  return encode_carve(nullptr, P, q);
}

extern "C" int skf_sketch_encode(const float* flat, long long P, const long long* offsets, int N, int mode, const double* centers,
                                 int K, int L, unsigned flags, void* out, float* scale, void* workspace, size_t workspace_bytes,
                                 skf_stream_t stream) {
  SKF_RAGGED_CHECK_ARGS(flat, P, offsets, N, workspace, workspace_bytes, skf_sketch_encode_workspace_bytes(P, N));
  SKF_CHECK_ARG(out, "null pointer");
  SKF_CHECK_ARG(L >= 2, "L must be at least 2");
  SKF_CHECK_ARG(mode == SKF_ENCODE_DICT || mode == SKF_ENCODE_GRID || mode == SKF_ENCODE_STROKE5, "mode must be DICT, GRID or STROKE5");
  SKF_CHECK_ARG((flags & ~(unsigned)SKF_ENCODE_CLAMP) == 0, "unknown flag");
  if (mode == SKF_ENCODE_DICT) {
    SKF_CHECK_ARG(centers != nullptr && ((uintptr_t)centers & 7) == 0, "DICT needs centers, 8-byte aligned");
    SKF_CHECK_ARG(K >= 1 && K <= TOK_MAXK, "K must be in [1, 4096]");
  } else if (mode == SKF_ENCODE_GRID) {
    SKF_CHECK_ARG(K >= 2 && K <= 32768 && K % 2 == 0, "the grid resolution must be even, in [2, 32768]");
  }
  SKF_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)scale & 3) == 0, "out, scale must be aligned to their element");
  hipStream_t st = (hipStream_t)stream;
  EncodeParams q;
  q.flat = flat; q.offsets = offsets; q.P = P; q.N = N; q.mode = mode; q.K = K; q.L = L; q.clamp = (flags & SKF_ENCODE_CLAMP) ? 1 : 0;
  q.out = out; q.scale = scale;
  encode_carve(workspace, P, q);

  const long long elems = (long long)N * L * (mode == SKF_ENCODE_STROKE5 ? 5 : 1);
  const long long fill_blocks = (elems + PACK_THREADS - 1) / PACK_THREADS;
  hipLaunchKernelGGL(encode_fill_kernel, dim3((unsigned)(fill_blocks < 65536 ? fill_blocks : 65536)), dim3(PACK_THREADS), 0, st, out, elems,
                     mode == SKF_ENCODE_STROKE5 ? 1 : 0);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(encode_scan_kernel, dim3(skf_cdiv(N, SCAN_THREADS)), dim3(SCAN_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  if (mode == SKF_ENCODE_DICT) {
    nearest_center_launch((const float*)q.xy, 2, P, centers, K, (int*)q.ids, st);
    SKF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(encode_pack_kernel, dim3((unsigned)((P + PACK_THREADS - 1) / PACK_THREADS)), dim3(PACK_THREADS), 0, st, q);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
