// Latent interpolation between pairs of embeddings (include/skf.h: skf_interpolate_f32): slerp (utils/skt_tools.py:18-25 of the
// reference) and lerp (:28-30), T steps per pair in one launch.  DESIGN.md section 3h.
//
// One wave per pair, four pairs per workgroup, no workspace:
//   1. lanes stride the two rows with 16-byte loads and accumulate |a|^2, |b|^2 and a.b in fp64 - the product of two fp32 values
//      is exact there - all three over the same elements in the same order, then through the same xor butterfly.  b = s a with s
//      a power of two therefore gives ab = s aa and bb = s^2 aa exactly, the cosine is exactly 1 and the pair takes the
//      "same direction" branch like the reference's `return p0`.
//   2. lane j (+ 64, ...) turns step t_j into the two fp32 weights, once per pair, and leaves them in the wave's slice of LDS.
//   3. every lane writes its columns of the T output rows: out = fmaf(w1, b, w0 * a), 16-byte stores.
#include "skf_common.h"

namespace {

constexpr int ITP_THREADS = 256;
constexpr int ITP_PAIRS = ITP_THREADS / SKF_WAVE;      // pairs per workgroup
constexpr int ITP_MAXT = 256;
constexpr int ITP_MAXD = 4096;

__global__ __launch_bounds__(ITP_THREADS) void interpolate_kernel(const float* a, int lda, const float* b, int ldb, int P, int d,
                                                                  const float* t, int T, int mode, float* out, int ldo) {
  __shared__ float sW[ITP_PAIRS][2 * ITP_MAXT];         // [w0 of the T steps | w1 of the T steps] per wave
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long pair = (long)blockIdx.x * ITP_PAIRS + w;
  const bool valid = pair < P;                          // waves behind P load and store nothing, but reach the barrier
  const float* ar = a + (size_t)(valid ? pair : 0) * lda;
  const float* br = b + (size_t)(valid ? pair : 0) * ldb;

  bool copy = false;                                    // every row of the pair is a[p] (wave-uniform)
  if (valid) {
    if (mode == 0) {
      double aa = 0.0, bb = 0.0, ab = 0.0;
      for (int c = lane * 4; c < d; c += 256) {
        const float4 x = *(const float4*)(ar + c), y = *(const float4*)(br + c);
        const double x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w, y0 = y.x, y1 = y.y, y2 = y.z, y3 = y.w;
        aa = fma(x0, x0, aa); bb = fma(y0, y0, bb); ab = fma(x0, y0, ab);
        aa = fma(x1, x1, aa); bb = fma(y1, y1, bb); ab = fma(x1, y1, ab);
        aa = fma(x2, x2, aa); bb = fma(y2, y2, bb); ab = fma(x2, y2, ab);
        aa = fma(x3, x3, aa); bb = fma(y3, y3, bb); ab = fma(x3, y3, ab);
      }
      aa = wave_sum(aa); bb = wave_sum(bb); ab = wave_sum(ab);
      // the reference takes arccos of the unclamped dot product of the normalised rows (NaN once rounding pushes it past 1);
      // clamped, those pairs land in the branch below
      const double cs = fmin(1.0, fmax(-1.0, ab / sqrt(aa * bb)));
      const double omega = acos(cs), so = sin(omega);
      copy = so < 1e-6;                                 // same or opposite direction: the reference's `return p0`
      if (!copy) {
        for (int j = lane; j < T; j += 64) {
          const double tj = (double)t[j];
          sW[w][j] = (float)(sin((1.0 - tj) * omega) / so);
          sW[w][T + j] = (float)(sin(tj * omega) / so);
        }
      }
    } else {
      for (int j = lane; j < T; j += 64) {
        const float tj = t[j];
        sW[w][j] = 1.0f - tj;
        sW[w][T + j] = tj;
      }
    }
  }
  __syncthreads();
  if (!valid) return;

  float* orow = out + (size_t)pair * T * ldo;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 x = *(const float4*)(ar + c), y = *(const float4*)(br + c);
    for (int j = 0; j < T; ++j) {
      float4 r = x;
      if (!copy) {
        const float w0 = sW[w][j], w1 = sW[w][T + j];
        r.x = fmaf(w1, y.x, w0 * x.x); r.y = fmaf(w1, y.y, w0 * x.y);
        r.z = fmaf(w1, y.z, w0 * x.z); r.w = fmaf(w1, y.w, w0 * x.w);
      }
      *(float4*)(orow + (size_t)j * ldo + c) = r;
    }
  }
}

}  // namespace

extern "C" int skf_interpolate_f32(const float* a, int lda, const float* b, int ldb, int P, int d, const float* t, int T, int mode,
                                   float* out, int ldo, skf_stream_t stream) {
  SKF_CHECK_ARG(a && b && t && out, "null pointer");
  SKF_CHECK_ARG(P >= 1, "P must be at least 1");
  SKF_CHECK_ARG(d >= 4 && d <= ITP_MAXD && d % 4 == 0, "d must be a multiple of 4 in [4, 4096]");
  SKF_CHECK_ARG(T >= 1 && T <= ITP_MAXT, "T must be in [1, 256]");
  SKF_CHECK_ARG((long long)P * T < (1ll << 31), "P * T must stay below 2^31 output rows");
  SKF_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (slerp) or 1 (lerp)");
  SKF_CHECK_ARG(lda >= d && ldb >= d && ldo >= d && lda % 4 == 0 && ldb % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)a & 15) == 0 &&
                    ((uintptr_t)b & 15) == 0 && ((uintptr_t)out & 15) == 0,
                "rows must be 16-byte aligned (base pointers and row pitches)");
  SKF_CHECK_ARG(((uintptr_t)t & 3) == 0, "t must be 4-byte aligned");
  hipLaunchKernelGGL(interpolate_kernel, dim3(skf_cdiv(P, ITP_PAIRS)), dim3(ITP_THREADS), 0, (hipStream_t)stream, a, lda, b, ldb, P, d,
                     t, T, mode, out, ldo);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
