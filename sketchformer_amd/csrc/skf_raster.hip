// Sketches as images (include/skf.h: skf_sketch_points, skf_rasterize_f32, skf_raster_overlap_f32).  DESIGN.md section 3l.
//
// skf_sketch_points: one wave per sketch walks its positions 64 at a time.  A ballot of "this position is a point" and the
//   pop-count of the lanes below give every point its place in the output (the compaction); the offsets of the kept lanes go
//   through a shuffle scan and a carry that the wave hands from chunk to chunk (the running sum); the pen of a point is the OR of
//   its own flag and "a separator lies between it and the next point", read off the two ballots.  The pen of the LAST point of a
//   chunk is held back in a register until the next point or the end of the sketch settles it, so no byte is written twice.
// skf_rasterize_f32: one workgroup per (32 x 32 pixel tile, sketch), 256 threads, four pixels each (rows y, y + 8, y + 16,
//   y + 24 of the tile: a wave stores two runs of 32 consecutive floats per row pair).  The points are walked in chunks of 256:
//   thread j builds primitive c0 + j in pixel space - a, b - a, 1 / |b - a|^2 - and tests its bounding box against the tile box
//   grown by line_width / 2 + 0.5 (a pixel further than that from every point of the primitive has coverage 0); the survivors
//   are compacted with a ballot per wave into an LDS list, and every thread walks that list.  All lanes read the same LDS
//   address in an iteration (a broadcast: no bank conflict) and every trip count is uniform over the workgroup.  The minimum of
//   the SQUARED distance is kept, one square root per pixel at the end.  No atomics, no workspace.
// skf_raster_overlap_f32: one workgroup per pair, fixed summation order (thread-strided partial sums, xor butterfly, the wave
//   sums added in wave order).
#include "skf_common.h"

namespace {

constexpr int PTS_STROKE3 = SKF_SKETCH_STROKE3, PTS_STROKE5 = SKF_SKETCH_STROKE5, PTS_DICT = SKF_SKETCH_DICT_TOKENS,
              PTS_GRID = SKF_SKETCH_GRID_TOKENS;

__global__ __launch_bounds__(SKF_WAVE) void sketch_points_kernel(int kind, const void* data, long ld, const int* lengths,
                                                                 const float* centers, int K, int T, float* xy, unsigned char* pen,
                                                                 int* n_points, float* bounds) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* fsrc = (const float*)data + (size_t)b * ld;
  const long long* tsrc = (const long long*)data + (size_t)b * ld;
  float* oxy = xy + (size_t)b * T * 2;
  unsigned char* open = pen + (size_t)b * T;
  const int len = kind == PTS_STROKE3 ? min(max(lengths[b], 0), T) : T;
  const long long nid = kind == PTS_GRID ? (long long)K * K : (long long)K;      // ids 1 .. nid name a point
  const double rhalf = (double)(K / 2);

  int n = 0;                         // points written so far (wave-uniform, like everything carried from chunk to chunk)
  float cx = 0.f, cy = 0.f;          // running position
  int held_pen = 0;                  // pen of point n - 1, not written yet
  bool done = false;
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;

  for (int t0 = 0; t0 < len && !done; t0 += SKF_WAVE) {
    const int t = t0 + lane;
    bool pt = false, sep = false, end = false;
    int own = 0;
    float ox = 0.f, oy = 0.f;
    if (t < len) {
      if (kind == PTS_STROKE3) {
        const float* r = fsrc + (size_t)t * 3;
        pt = true; ox = r[0]; oy = r[1]; own = r[2] == 1.0f;
      } else if (kind == PTS_STROKE5) {
        const float* r = fsrc + (size_t)t * 5;
        int a = 0;                                      // argmax of r[2:5], ties to the first index
        float m = r[2];
        if (r[3] > m) { m = r[3]; a = 1; }
        if (r[4] > m) a = 2;
        end = a == 2; pt = !end; own = a == 1; ox = r[0]; oy = r[1];
      } else {
        const long long id = tsrc[t];
        pt = id >= 1 && id <= nid;                      // an id outside the vocabulary is neither of the three: skipped
        sep = id == nid + 1;
        end = id == nid + 3;
        if (pt && kind == PTS_DICT) {
          ox = centers[2 * (id - 1)]; oy = centers[2 * (id - 1) + 1];
        } else if (pt) {                                // the cell centre, in the host decoder's fp64 expression
          const long long c = (id - 1) % K, r = (id - 1) / K;
          ox = (float)((double)c / rhalf - 1.0 + 1.0 / (double)K);
          oy = (float)((double)r / rhalf - 1.0 + 1.0 / (double)K);
        }
      }
    }
    const unsigned long long endm = __ballot(end);
    const unsigned long long live = endm ? ((endm & (0ull - endm)) - 1ull) : ~0ull;      // the lanes before the first end
    done = endm != 0ull;
    const unsigned long long ptm = __ballot(pt) & live, sepm = __ballot(sep) & live;
    pt = (ptm >> lane) & 1ull;
    if (!pt) { ox = 0.f; oy = 0.f; }

    float px = ox, py = oy;
    if (kind != PTS_GRID) {                             // offsets: inclusive scan over the wave + the carry
#pragma unroll
      for (int o = 1; o < SKF_WAVE; o <<= 1) {
        const float ux = __shfl_up(px, o, SKF_WAVE), uy = __shfl_up(py, o, SKF_WAVE);
        if (lane >= o) { px += ux; py += uy; }
      }
      px += cx; py += cy;
      cx = __shfl(px, SKF_WAVE - 1, SKF_WAVE); cy = __shfl(py, SKF_WAVE - 1, SKF_WAVE);
    }

    const unsigned long long above = lane == SKF_WAVE - 1 ? 0ull : (~0ull << (lane + 1));
    const unsigned long long nextm = ptm & above;
    const unsigned long long upto = nextm ? ((nextm & (0ull - nextm)) - 1ull) : ~0ull;   // the lanes below the next point
    const int p = own | ((sepm & above & upto) != 0ull);
    const int first = ptm ? __ffsll((long long)ptm) - 1 : SKF_WAVE;
    const unsigned long long lead = first == SKF_WAVE ? sepm : (sepm & ((1ull << first) - 1ull));
    if (n > 0 && lead) held_pen = 1;                    // separators in front of the chunk's first point lift the pen of point n - 1
    if (ptm) {
      const int last = 63 - __clzll((long long)ptm);
      if (n > 0 && lane == 0) open[n - 1] = (unsigned char)held_pen;
      if (pt) {
        const int idx = n + __popcll(ptm & ((1ull << lane) - 1ull));       // idx <= t < T
        oxy[2 * idx] = px; oxy[2 * idx + 1] = py;
        if (lane != last) open[idx] = (unsigned char)p;
        mnx = fminf(mnx, px); mny = fminf(mny, py); mxx = fmaxf(mxx, px); mxy = fmaxf(mxy, py);
      }
      held_pen = __shfl(p, last, SKF_WAVE);
      n += __popcll(ptm);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mnx = fminf(mnx, __shfl_xor(mnx, o, SKF_WAVE)); mny = fminf(mny, __shfl_xor(mny, o, SKF_WAVE));
    mxx = fmaxf(mxx, __shfl_xor(mxx, o, SKF_WAVE)); mxy = fmaxf(mxy, __shfl_xor(mxy, o, SKF_WAVE));
  }
  if (lane == 0) {
    if (n > 0) open[n - 1] = (unsigned char)(kind == PTS_GRID ? 1 : held_pen);      // the grid decoder closes its last line
    n_points[b] = n;
    float* bo = bounds + (size_t)b * 4;
    bo[0] = n ? mnx : 0.f; bo[1] = n ? mny : 0.f; bo[2] = n ? mxx : 0.f; bo[3] = n ? mxy : 0.f;
  }
  for (int i = n + lane; i < T; i += SKF_WAVE) {        // the rows behind the sketch: zeros
    oxy[2 * i] = 0.f; oxy[2 * i + 1] = 0.f; open[i] = 0;
  }
}

constexpr int RAS_THREADS = 256;
constexpr int RAS_WAVES = RAS_THREADS / SKF_WAVE;
constexpr int RAS_TW = 32, RAS_TH = 32;                 // pixel tile of a workgroup
constexpr int RAS_PIX = RAS_TW * RAS_TH / RAS_THREADS;  // pixels per thread
constexpr int RAS_ROWSTEP = RAS_THREADS / RAS_TW;

__global__ __launch_bounds__(RAS_THREADS) void rasterize_kernel(const float* xy, const unsigned char* pen, const int* n_points,
                                                                const float* frames, int T, int H, int W, int tiles_x, int tiles_y,
                                                                float line_width, float margin, float* out) {
  __shared__ float4 sSeg[RAS_THREADS];                  // a.x, a.y, (b - a).x, (b - a).y of the chunk's survivors
  __shared__ float sInv[RAS_THREADS];                   // 1 / |b - a|^2 (0 for a dot)
  __shared__ int sCount[RAS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tile = blockIdx.x % (tiles_x * tiles_y), b = blockIdx.x / (tiles_x * tiles_y);
  const int tx0 = (tile % tiles_x) * RAS_TW, ty0 = (tile / tiles_x) * RAS_TH;
  const float* pxy = xy + (size_t)b * T * 2;
  const unsigned char* ppen = pen + (size_t)b * T;
  const int n = min(max(n_points[b], 0), T);

  // the frame: pixel = (W / 2, H / 2) + s (p - box centre)
  const float* fr = frames + (size_t)b * 4;
  const float bw = fr[2] - fr[0], bh = fr[3] - fr[1];
  const float fx = ((float)W - 2.f * margin) / bw, fy = ((float)H - 2.f * margin) / bh;
  const bool hasw = bw >= 1e-6f, hash = bh >= 1e-6f;
  const float s = hasw ? (hash ? fminf(fx, fy) : fx) : (hash ? fy : 0.f);
  const float bcx = 0.5f * (fr[0] + fr[2]), bcy = 0.5f * (fr[1] + fr[3]);
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;

  const float grow = 0.5f * line_width + 0.5f;
  const float bx0 = ((float)tx0 - hw) - grow, bx1 = ((float)(tx0 + RAS_TW) - hw) + grow;
  const float by0 = ((float)ty0 - hh) - grow, by1 = ((float)(ty0 + RAS_TH) - hh) + grow;

  // points and pixel centres are both taken relative to the canvas centre: the same distances from coordinates half as large
  const int u = tx0 + (tid & (RAS_TW - 1)), v0 = ty0 + tid / RAS_TW;
  const float pcx = ((float)u + 0.5f) - hw;
  float best[RAS_PIX], pcy[RAS_PIX];
#pragma unroll
  for (int k = 0; k < RAS_PIX; ++k) {
    best[k] = 3.0e38f;
    pcy[k] = ((float)(v0 + k * RAS_ROWSTEP) + 0.5f) - hh;
  }

  for (int c0 = 0; c0 < n; c0 += RAS_THREADS) {         // n is uniform over the workgroup
    const int i = c0 + tid;
    bool keep = false;
    float ax = 0.f, ay = 0.f, dx = 0.f, dy = 0.f, inv = 0.f;
    if (i < n) {
      const float qx = s * (pxy[2 * i] - bcx), qy = s * (pxy[2 * i + 1] - bcy);
      ax = qx; ay = qy;
      if (i > 0 && ppen[i - 1] == 0) {
        ax = s * (pxy[2 * i - 2] - bcx); ay = s * (pxy[2 * i - 1] - bcy);
      }
      dx = qx - ax; dy = qy - ay;
      const float l2 = dx * dx + dy * dy;
      inv = l2 > 0.f ? 1.0f / l2 : 0.f;
      keep = fmaxf(ax, qx) >= bx0 && fminf(ax, qx) <= bx1 && fmaxf(ay, qy) >= by0 && fminf(ay, qy) <= by1;
    }
    const unsigned long long km = __ballot(keep);
    if (lane == 0) sCount[wv] = __popcll(km);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RAS_WAVES; ++w) {
      const int c = sCount[w];
      if (w < wv) base += c;
      total += c;
    }
    if (keep) {
      const int slot = base + __popcll(km & ((1ull << lane) - 1ull));
      sSeg[slot] = make_float4(ax, ay, dx, dy);
      sInv[slot] = inv;
    }
    __syncthreads();
    for (int j = 0; j < total; ++j) {
      const float4 sg = sSeg[j];
      const float iv = sInv[j];
      const float rx = pcx - sg.x;
#pragma unroll
      for (int k = 0; k < RAS_PIX; ++k) {
        const float ry = pcy[k] - sg.y;
        const float tt = fminf(fmaxf((rx * sg.z + ry * sg.w) * iv, 0.f), 1.f);
        // one fused multiply-add each: t (b - a) is as long as the segment, e as short as the distance
        const float ex = fmaf(-tt, sg.z, rx), ey = fmaf(-tt, sg.w, ry);
        best[k] = fminf(best[k], ex * ex + ey * ey);
      }
    }
    __syncthreads();                                    // the list is rewritten by the next chunk
  }

  if (u < W) {
    float* o = out + (size_t)b * H * W;
#pragma unroll
    for (int k = 0; k < RAS_PIX; ++k) {
      const int v = v0 + k * RAS_ROWSTEP;
      if (v < H) o[(size_t)v * W + u] = fminf(fmaxf(0.5f + 0.5f * line_width - sqrtf(best[k]), 0.f), 1.f);
    }
  }
}

constexpr int OVL_THREADS = 1024;

__global__ __launch_bounds__(OVL_THREADS) void raster_overlap_kernel(const float* a, long lda, const float* b, long ldb, long N,
                                                                     float* out) {
  __shared__ float sMin[OVL_THREADS / SKF_WAVE], sMax[OVL_THREADS / SKF_WAVE];
  const float* ar = a + (size_t)blockIdx.x * lda;
  const float* br = b + (size_t)blockIdx.x * ldb;
  float lo = 0.f, hi = 0.f;
  long i = threadIdx.x;
  for (; i + 3 * OVL_THREADS < N; i += 4 * OVL_THREADS) {      // four independent loads of each row in flight
    const float x0 = ar[i], x1 = ar[i + OVL_THREADS], x2 = ar[i + 2 * OVL_THREADS], x3 = ar[i + 3 * OVL_THREADS];
    const float y0 = br[i], y1 = br[i + OVL_THREADS], y2 = br[i + 2 * OVL_THREADS], y3 = br[i + 3 * OVL_THREADS];
    lo += (fminf(x0, y0) + fminf(x1, y1)) + (fminf(x2, y2) + fminf(x3, y3));
    hi += (fmaxf(x0, y0) + fmaxf(x1, y1)) + (fmaxf(x2, y2) + fmaxf(x3, y3));
  }
  for (; i < N; i += OVL_THREADS) {
    const float x = ar[i], y = br[i];
    lo += fminf(x, y); hi += fmaxf(x, y);
  }
  lo = wave_sum(lo); hi = wave_sum(hi);
  if ((threadIdx.x & 63) == 0) { sMin[threadIdx.x >> 6] = lo; sMax[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float l = sMin[0], h = sMax[0];
    for (int w = 1; w < OVL_THREADS / SKF_WAVE; ++w) { l += sMin[w]; h += sMax[w]; }
    out[2 * (size_t)blockIdx.x] = l; out[2 * (size_t)blockIdx.x + 1] = h;
  }
}

}  // namespace

extern "C" int skf_sketch_points(int kind, const void* data, long long ld, const int* lengths, const float* centers, int K, int B,
                                 int T, float* xy, unsigned char* pen, int* n_points, float* bounds, skf_stream_t stream) {
  SKF_CHECK_ARG(kind >= PTS_STROKE3 && kind <= PTS_GRID, "kind must be 0 (stroke-3), 1 (stroke-5), 2 (dictionary tokens) or 3 (grid tokens)");
  SKF_CHECK_ARG(data && xy && pen && n_points && bounds, "null pointer");
  SKF_CHECK_ARG(B >= 1 && T >= 1, "B and T must be at least 1");
  SKF_CHECK_ARG((long long)T * 5 < (1ll << 31), "T must stay below 2^31 / 5 positions");
  const int width = kind == PTS_STROKE3 ? 3 : kind == PTS_STROKE5 ? 5 : 1;
  SKF_CHECK_ARG(ld >= (long long)T * width, "ld must hold the T positions of a sketch");
  SKF_CHECK_ARG(((uintptr_t)data & (kind >= PTS_DICT ? 7 : 3)) == 0, "data must be aligned to its element size");
  if (kind == PTS_STROKE3) SKF_CHECK_ARG(lengths != nullptr, "stroke-3 needs lengths");
  if (kind == PTS_DICT) SKF_CHECK_ARG(centers != nullptr && K >= 1, "dictionary tokens need centers (K, 2), K >= 1");
  if (kind == PTS_GRID) SKF_CHECK_ARG(K >= 2 && K % 2 == 0 && K <= 32768, "the grid resolution must be even, in [2, 32768]");
  SkfProfScope ps_((hipStream_t)stream, "sketch_points", 0.0, (double)B * T * (width * (kind >= PTS_DICT ? 8.0 : 4.0) + 9.0));
  hipLaunchKernelGGL(sketch_points_kernel, dim3(B), dim3(SKF_WAVE), 0, (hipStream_t)stream, kind, data, (long)ld, lengths, centers, K, T,
                     xy, pen, n_points, bounds);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_rasterize_f32(const float* xy, const unsigned char* pen, const int* n_points, const float* frames, int B, int T,
                                 int H, int W, float line_width, float margin, float* out, skf_stream_t stream) {
  SKF_CHECK_ARG(xy && pen && n_points && frames && out, "null pointer");
  SKF_CHECK_ARG(B >= 1 && T >= 1, "B and T must be at least 1");
  SKF_CHECK_ARG(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "H and W must be in [1, 16384]");
  SKF_CHECK_ARG(line_width > 0.f && line_width <= 1024.f, "line_width must be in (0, 1024]");
  SKF_CHECK_ARG(margin >= 0.f && 2.f * margin < (float)(H < W ? H : W), "margin must be >= 0 and 2 * margin < min(H, W)");
  const int tiles_x = skf_cdiv(W, RAS_TW), tiles_y = skf_cdiv(H, RAS_TH);
  SKF_CHECK_ARG((long long)tiles_x * tiles_y * B < (1ll << 31), "tiles * B must stay below 2^31 workgroups");
  SkfProfScope ps_((hipStream_t)stream, "rasterize", 0.0, 4.0 * B * H * W);
  hipLaunchKernelGGL(rasterize_kernel, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(RAS_THREADS), 0, (hipStream_t)stream, xy, pen, n_points,
                     frames, T, H, W, tiles_x, tiles_y, line_width, margin, out);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_raster_overlap_f32(const float* a, long long lda, const float* b, long long ldb, int B, long long N, float* out,
                                      skf_stream_t stream) {
  SKF_CHECK_ARG(a && b && out, "null pointer");
  SKF_CHECK_ARG(B >= 1 && N >= 1, "B and N must be at least 1");
  SKF_CHECK_ARG(lda >= N && ldb >= N, "lda and ldb must be at least N");
  SkfProfScope ps_((hipStream_t)stream, "raster_overlap", 2.0 * B * N, 8.0 * B * N);
  hipLaunchKernelGGL(raster_overlap_kernel, dim3(B), dim3(OVL_THREADS), 0, (hipStream_t)stream, a, (long)lda, b, (long)ldb, (long)N, out);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
