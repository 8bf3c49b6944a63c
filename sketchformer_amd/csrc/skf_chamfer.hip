// Order-free shape distances on the device (include/skf.h: skf_shape_distance_f32): the directed mean and the directed maximum of
// the nearest-ink distance between two sketches, both ways, from which the Python layer takes the Chamfer and the Hausdorff
// distance.  The reference has nothing in their place; the specification is the rule of include/skf.h, restated in float32 numpy
// by tests/shape_reference.py, which the kernel matches bit for bit.  DESIGN.md section 3s.
//
// Work split.  A workgroup of four waves keeps ONE sketch A resident in LDS - per point i its position p[i], the edge
// e = p[i] - p[i-1] of the segment that ends there, 1 / |e|^2 and a segment flag - and walks a block of SD_GALLERY_BLOCK rows of b
// (cross mode; one row in paired mode), staging each the same way.  With both sketches resident both directions of the pair are
// computed: a lane owns sample slots of one sketch, (point i, step j) for j < S, and walks ALL primitives of the other sketch with
// a running minimum in a register.  Every lane of the workgroup reads the same primitive at the same time, so the LDS reads are
// broadcasts; the (samples x primitives) table never exists.  Two slots per lane share one walk while a pass has work for both.
//
// One walk step serves a dot and a segment.  Step k of a walk evaluates the dot p[k] and the segment p[k-1] -> p[k].  The
// vector s - p[k-1] the segment needs is the vector the dot of step k - 1 just used, so it is carried in registers.  Where point k
// ends no segment (a pen lift in front of it, k = 0, a repeated point), e and inv are stored as zeros: t clamps to 0 and the
// segment expression returns |s - p[k-1]|^2, the value of a dot that is in the minimum anyway, bit for bit.  The loop therefore
// has no branch, and the minimum is the one the rule defines.
//
// Exactness.  -ffp-contract=off (build.SOURCE_FLAGS) and the pragma below keep every multiply and add rounded on its own; 1 / len2,
// j / S and the square root are hipcc's correctly rounded defaults.  min and max are exact and the mean is an int64 fixed-point
// sum, so neither the split of the samples over lanes nor the order of the reduction can change a bit.  The clamp of t is one
// v_med3 / clamp modifier: equal to min(max(x, 0), 1) for every x that is not a NaN (finite inputs are the caller's contract).
// -fno-slp-vectorize as for skf_kmeans.hip: left alone, -O3 pairs the x and y halves of the walk into v_pk_*_f32, which gain
// nothing over two scalar instructions on gfx950 and add moves.
// Registers and LDS as compiled: profiles/chamfer_build.txt.
#include "skf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SD_WAVES = 4;
constexpr int SD_THREADS = SD_WAVES * SKF_WAVE;
constexpr int SD_GALLERY_BLOCK = 8;                               // rows of b per workgroup in cross mode (ops.SHAPE_GALLERY_BLOCK)
constexpr int SD_MAX_S = 16;

struct Sketch {                                                   // one resident sketch: 10.5 KiB of LDS
  float4 pe[SKF_ALIGN_MAX_LEN];                                   // (p.x, p.y, e.x, e.y); e = 0 where no segment ends
  float inv[SKF_ALIGN_MAX_LEN];                                   // 1 / |e|^2, or 0
  unsigned char seg[SKF_ALIGN_MAX_LEN];                           // 1: a segment ends at this point (it adds S - 1 samples)
};

struct Acc {                                                      // one direction of one pair, per lane
  long long q;                                                    // sum of floor(d * 2^24)
  float mx;
  int cnt;
};

// row -> LDS by the whole workgroup.  n is clamped by the caller; an empty sketch becomes the single point (0, 0).  -> points held
__device__ __forceinline__ int stage(Sketch& s, const float* __restrict__ xy, const unsigned char* __restrict__ pen, int n) {
  const int L = n < 1 ? 1 : n;
  for (int i = threadIdx.x; i < L; i += SD_THREADS) {
    const bool real = i < n, seg = real && i > 0 && pen[i - 1] == 0;
    const float px = real ? xy[2 * i] : 0.0f, py = real ? xy[2 * i + 1] : 0.0f;
    float ex = 0.0f, ey = 0.0f, inv = 0.0f;
    if (seg) {
      ex = px - xy[2 * i - 2];
      ey = py - xy[2 * i - 1];
      const float len2 = ex * ex + ey * ey;
      inv = len2 > 0.0f ? 1.0f / len2 : 0.0f;
    }
    s.pe[i] = make_float4(px, py, ex, ey);
    s.inv[i] = inv;
    s.seg[i] = seg ? 1 : 0;
  }
  return L;
}

// the squared distance of U samples to every primitive of Y: the minimum
template <int U>
__device__ __forceinline__ void nearest(const Sketch& Y, int Ly, const float (&sx)[2], const float (&sy)[2], float (&best)[2]) {
  float qx[U], qy[U], m[U];
  const float4 first = Y.pe[0];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    qx[u] = sx[u] - first.x;
    qy[u] = sy[u] - first.y;
    m[u] = __builtin_inff();
  }
  for (int k = 0; k < Ly; ++k) {
    const float4 v = Y.pe[k];
    const float inv = Y.inv[k];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float px = qx[u], py = qy[u];                         // s - p[k - 1]: the segment's start
      const float dot = px * v.z + py * v.w;
      const float t = __builtin_amdgcn_fmed3f(dot * inv, 0.0f, 1.0f);
      const float rx = px - t * v.z, ry = py - t * v.w;
      const float d_seg = rx * rx + ry * ry;
      qx[u] = sx[u] - v.x;
      qy[u] = sy[u] - v.y;
      const float d_dot = qx[u] * qx[u] + qy[u] * qy[u];
      m[u] = fminf(m[u], fminf(d_seg, d_dot));
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) best[u] = m[u];
}

// every sample of X against Y.  Slots (i, j), j < S: j = 0 is the point p[i] itself, j > 0 the sample p[i-1] + (j / S) e of the
// segment that ends at i, if one does.
__device__ __forceinline__ void directed(const Sketch& X, int Lx, const Sketch& Y, int Ly, int S, const float* tS, Acc& acc) {
  const int nslots = Lx * S;
  for (int base = 0; base < nslots; base += 2 * SD_THREADS) {
    float sx[2], sy[2], best[2] = {0.0f, 0.0f};
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int slot = base + u * SD_THREADS + (int)threadIdx.x;
      const int i = min(slot / S, Lx - 1), j = slot % S;          // (clamped: a slot behind the end indexes point Lx - 1)
      ok[u] = slot < nslots && (j == 0 || X.seg[i] != 0);
      const bool inner = ok[u] && j > 0;                          // (then i > 0)
      const float4 v = X.pe[ok[u] ? i : 0];
      const float4 a = X.pe[inner ? i - 1 : 0];
      const float t = tS[inner ? j : 0];
      const float ix = a.x + t * v.z, iy = a.y + t * v.w;
      sx[u] = inner ? ix : v.x;                                   // a point is used as it is, never recomputed
      sy[u] = inner ? iy : v.y;
    }
    // wave-uniform: a wave whose slots are all behind the end, or all on points that end no segment, has nothing to walk
    const bool any0 = __any(ok[0]), any1 = __any(ok[1]);
    if (any1) nearest<2>(Y, Ly, sx, sy, best);
    else if (any0) nearest<1>(Y, Ly, sx, sy, best);
    else continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (ok[u]) {                                                // (ok[1] is false in every lane of a wave that walked one slot)
        const float d = sqrtf(best[u]);                           // correctly rounded: hipcc's default for sqrtf
        acc.mx = fmaxf(acc.mx, d);
        acc.q += (long long)floor((double)d * 16777216.0);
        acc.cnt += 1;
      }
    }
  }
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SD_THREADS) void shape_distance_kernel(const float* __restrict__ xy_a, long long lda,
                                                                    const unsigned char* __restrict__ pen_a, long long ldpa,
                                                                    const int* __restrict__ n_a, int Na, int Ta,
                                                                    const float* __restrict__ xy_b, long long ldb,
                                                                    const unsigned char* __restrict__ pen_b, long long ldpb,
                                                                    const int* __restrict__ n_b, int Nb, int Tb, int S, int cross,
                                                                    int groups, float* __restrict__ out) {
  __shared__ Sketch sA, sB;
  __shared__ float tS[SD_MAX_S];
  __shared__ long long sQ[2][SD_WAVES];
  __shared__ float sM[2][SD_WAVES];
  __shared__ int sC[2][SD_WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the row of a and the rows of b of this workgroup (the grid is exact: ia < Na and jb0 < Nb)
  long long ia, jb0;
  int rows;
  if (cross) {
    ia = blockIdx.x / groups;
    jb0 = (long long)(blockIdx.x % groups) * SD_GALLERY_BLOCK;
    rows = (int)min((long long)SD_GALLERY_BLOCK, Nb - jb0);
  } else {
    ia = jb0 = blockIdx.x;
    rows = 1;
  }
  if (threadIdx.x < SD_MAX_S) tS[threadIdx.x] = (float)(int)threadIdx.x / (float)S;      // j / S, correctly rounded; j < S is read
  const int na = __builtin_amdgcn_readfirstlane(min(max(n_a[ia], 0), Ta));
  const int La = stage(sA, xy_a + (size_t)ia * lda, pen_a + (size_t)ia * ldpa, na);
  for (int r = 0; r < rows; ++r) {
    const long long jb = jb0 + r;
    const int nb = __builtin_amdgcn_readfirstlane(min(max(n_b[jb], 0), Tb));
    // (the waves that still walked the row before this one have met the barrier of its reduction)
    const int Lb = stage(sB, xy_b + (size_t)jb * ldb, pen_b + (size_t)jb * ldpb, nb);
    __syncthreads();
    Acc ab = {0ll, 0.0f, 0}, ba = {0ll, 0.0f, 0};
    directed(sA, La, sB, Lb, S, tS, ab);
    directed(sB, Lb, sA, La, S, tS, ba);
    const long long q0 = wave_sum_i64(ab.q), q1 = wave_sum_i64(ba.q);
    const float m0 = wave_max(ab.mx), m1 = wave_max(ba.mx);
    const int c0 = wave_sum_i32(ab.cnt), c1 = wave_sum_i32(ba.cnt);
    if (lane == 0) {
      sQ[0][wave] = q0; sQ[1][wave] = q1;
      sM[0][wave] = m0; sM[1][wave] = m1;
      sC[0][wave] = c0; sC[1][wave] = c1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                       // (read before this thread meets the next row's barrier)
      float mean[2], mx[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        long long q = 0;
        int c = 0;
        float m = 0.0f;
#pragma unroll
        for (int w = 0; w < SD_WAVES; ++w) {
          q += sQ[d][w];
          c += sC[d][w];
          m = fmaxf(m, sM[d][w]);
        }
        mean[d] = (float)(((double)q / 16777216.0) / (double)c);  // c >= 1: slot (0, 0) is always a sample
        mx[d] = m;
      }
      const size_t o = cross ? (size_t)ia * Nb + jb : (size_t)ia;
      reinterpret_cast<float4*>(out)[o] = make_float4(mean[0], mean[1], mx[0], mx[1]);
    }
  }
}

}  // namespace

extern "C" int skf_shape_distance_f32(const float* xy_a, long long lda, const unsigned char* pen_a, long long ldpa, const int* n_a, int Na,
                                      int Ta, const float* xy_b, long long ldb, const unsigned char* pen_b, long long ldpb, const int* n_b,
                                      int Nb, int Tb, int samples_per_segment, int cross, float* out, skf_stream_t stream) {
  SKF_CHECK_ARG(xy_a && pen_a && n_a && xy_b && pen_b && n_b && out, "null pointer");
  SKF_CHECK_ARG(Na >= 1 && Nb >= 1, "Na and Nb must be at least 1");
  SKF_CHECK_ARG(Ta >= 1 && Tb >= 1, "Ta and Tb must be at least 1");
  SKF_CHECK_ARG(Ta <= SKF_ALIGN_MAX_LEN && Tb <= SKF_ALIGN_MAX_LEN, "Ta and Tb must not exceed SKF_ALIGN_MAX_LEN");
  SKF_CHECK_ARG(lda >= 2ll * Ta && ldb >= 2ll * Tb, "a row stride of the points is shorter than its row");
  SKF_CHECK_ARG(ldpa >= Ta && ldpb >= Tb, "a row stride of the pen bytes is shorter than its row");
  SKF_CHECK_ARG(samples_per_segment >= 1 && samples_per_segment <= SD_MAX_S, "samples_per_segment must be in [1, 16]");
  SKF_CHECK_ARG(cross == 0 || cross == 1, "cross must be 0 or 1");
  SKF_CHECK_ARG(cross || Na == Nb, "paired mode needs Na == Nb");
  SKF_CHECK_ARG(!cross || (long long)Na * Nb * 4 < (1ll << 31), "the cross matrix must hold fewer than 2^31 floats");
  SKF_CHECK_ARG(((uintptr_t)xy_a & 3) == 0 && ((uintptr_t)xy_b & 3) == 0 && ((uintptr_t)n_a & 3) == 0 && ((uintptr_t)n_b & 3) == 0,
                "xy_a, xy_b and the lengths must be 4-byte aligned");
  SKF_CHECK_ARG(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
  const long long groups = (Nb + SD_GALLERY_BLOCK - 1) / SD_GALLERY_BLOCK;
  const long long blocks = cross ? (long long)Na * groups : (long long)Na;          // below 2^29: the check of the matrix above
  hipLaunchKernelGGL(shape_distance_kernel, dim3((unsigned)blocks), dim3(SD_THREADS), 0, (hipStream_t)stream, xy_a, lda, pen_a, ldpa, n_a,
                     Na, Ta, xy_b, ldb, pen_b, ldpb, n_b, Nb, Tb, samples_per_segment, cross, (int)groups, out);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
