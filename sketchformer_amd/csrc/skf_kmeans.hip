// Lloyd k-means for 2-D points (include/skf.h: skf_kmeans_assign_f32, skf_kmeans_step_f32): the fit behind the token dictionary
// of prep_data/sketch_token/create_token_dict.py.  DESIGN.md section 3g.
//
//   kmeans_assign_kernel<false>  labels (and distances) only
//   kmeans_assign_kernel<true>   the same assignment + per-centre count and coordinate sums + per-tile inertia partials
//   kmeans_update_kernel         one workgroup: new centres, shift, inertia, empty count, iteration count, the stop flag
//
// A workgroup stages all K centres in LDS once and walks tiles of 2048 points (8 per thread, in registers) in a grid-stride loop;
// every lane of a wave reads the same centre (an LDS broadcast), so a centre costs one ds_read for 8 x 64 point-centre pairs.
// The arithmetic is scalar fp32 VALU, not packed: MI355X_MICROARCH.md gives v_pk_fma_f32 and v_fma_f32 the same peak
// (64 FLOP/clk/SIMD), so packing buys no rate here, and only half of the seven instructions of a pair (two subtracts, multiply, fma,
// compare, two selects) have a packed form at all.
//
// Determinism.  The distance of a pair is fmaf(dy, dy, dx * dx) of dx = x - cx, dy = y - cy: one definition, no dependence on the
// launch geometry.  "d < best" over ascending centre indices keeps the FIRST minimum.  Counts and coordinate sums are integers
// (rint(x * 2^e) summed as 64-bit two's complement; LDS and global integer atomics commute), the inertia is summed in fp64 in a fixed
// order: per thread over its 8 points, xor butterfly over the wave, waves in order, tiles in order - the tile, not the workgroup, owns
// a partial, so the grid size does not enter.  No floating-point atomic anywhere.
#include "skf_common.h"

namespace {

typedef unsigned long long u64;
constexpr int KM_THREADS = 256;
constexpr int KM_PPT = 8;                         // points per thread
constexpr int KM_TILE = KM_THREADS * KM_PPT;      // points per tile
constexpr int KM_MAXK = 4096;
constexpr int KM_MAXGRID = 1024;                  // 4 resident workgroups per CU at K = 1000 (28 KB of LDS each)

struct KmParams {
  const float* pts; const float* ctr; int* labels; float* dist;
  u64* sums; unsigned* counts; double* partials; const SkfKmeansState* state;
  long N; int ldp, ldc, K, ntiles; float scale;
};

template <bool ACC>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(KmParams p) {
  extern __shared__ __align__(16) unsigned char km_smem[];
  // [K (rounded up to even) float2 centres][ACC: 2 K u64 sums][ACC: K u32 counts][ACC: 4 doubles]
  const int Kp = (p.K + 1) & ~1;
  float2* sC = (float2*)km_smem;
  u64* sSum = (u64*)(km_smem + (size_t)Kp * 8);
  double* sRed = (double*)(sSum + 2 * (size_t)p.K);
  unsigned* sCnt = (unsigned*)(sRed + 4);
  const int tid = threadIdx.x;
  if (ACC && p.state->converged) return;          // the fit has stopped: this launch is a no-op (uniform over the grid)

  for (int k = tid; k < Kp; k += KM_THREADS)
    sC[k] = k < p.K ? *(const float2*)(p.ctr + (size_t)k * p.ldc) : make_float2(0.f, 0.f);
  if (ACC) {
    for (int k = tid; k < p.K; k += KM_THREADS) { sSum[2 * k] = 0; sSum[2 * k + 1] = 0; sCnt[k] = 0; }
  }
  __syncthreads();

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const long base = (long)tile * KM_TILE + tid;
    float x[KM_PPT], y[KM_PPT], best[KM_PPT];
    int idx[KM_PPT];
#pragma unroll
    for (int j = 0; j < KM_PPT; ++j) {
      const long i = base + (long)j * KM_THREADS;
      const float2 v = i < p.N ? *(const float2*)(p.pts + (size_t)i * p.ldp) : make_float2(0.f, 0.f);
      x[j] = v.x; y[j] = v.y; best[j] = __builtin_inff(); idx[j] = 0;
    }
#pragma unroll 4
    for (int k = 0; k < p.K; ++k) {
      const float2 c = sC[k];
#pragma unroll
      for (int j = 0; j < KM_PPT; ++j) {
        const float dx = x[j] - c.x, dy = y[j] - c.y;
        const float d = fmaf(dy, dy, dx * dx);
        const bool lt = d < best[j];              // strict: the lowest index among equal minima stays
        best[j] = lt ? d : best[j];
        idx[j] = lt ? k : idx[j];
      }
    }
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < KM_PPT; ++j) {
      const long i = base + (long)j * KM_THREADS;
      if (i < p.N) {
        p.labels[i] = idx[j];
        if (p.dist) p.dist[i] = best[j];
        if (ACC) {
          const long long qx = (long long)__float2int_rn(x[j] * p.scale), qy = (long long)__float2int_rn(y[j] * p.scale);
          atomicAdd(&sCnt[idx[j]], 1u);
          atomicAdd(&sSum[2 * idx[j]], (u64)qx);
          atomicAdd(&sSum[2 * idx[j] + 1], (u64)qy);
          part += (double)best[j];
        }
      }
    }
    if (ACC) {
      part = block_sum(part, sRed);
      if (tid == 0) p.partials[tile] = part;
    }
  }

  if (ACC) {
    __syncthreads();
    for (int k = tid; k < p.K; k += KM_THREADS) {
      const unsigned n = sCnt[k];
      if (n) {
        atomicAdd(&p.counts[k], n);
        atomicAdd(&p.sums[2 * k], sSum[2 * k]);
        atomicAdd(&p.sums[2 * k + 1], sSum[2 * k + 1]);
      }
    }
  }
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(float* ctr, int ldc, int K, const u64* sums, const unsigned* counts,
                                                                   const double* partials, int ntiles, double inv_scale, double tol_abs,
                                                                   int* counts_out, SkfKmeansState* state) {
  __shared__ double sRed[4];
  if (state->converged) return;
  const int tid = threadIdx.x;
  double shift = 0.0, inertia = 0.0, empty = 0.0;
  for (int k = tid; k < K; k += KM_THREADS) {
    const unsigned n = counts[k];
    if (counts_out) counts_out[k] = (int)n;
    if (n == 0) { empty += 1.0; continue; }       // a centre without points keeps its coordinates
    float* c = ctr + (size_t)k * ldc;
    // the mean in fp64 from the integer sums, rounded once to fp32
    const float nx = (float)((double)(long long)sums[2 * k] / (double)n * inv_scale);
    const float ny = (float)((double)(long long)sums[2 * k + 1] / (double)n * inv_scale);
    const double ddx = (double)nx - (double)c[0], ddy = (double)ny - (double)c[1];
    shift += ddx * ddx + ddy * ddy;
    c[0] = nx; c[1] = ny;
  }
  for (int t = tid; t < ntiles; t += KM_THREADS) inertia += partials[t];
  shift = block_sum(shift, sRed);
  inertia = block_sum(inertia, sRed);
  empty = block_sum(empty, sRed);
  if (tid == 0) {
    state->iterations += 1;
    state->n_empty = (int)empty;
    state->inertia = inertia;
    state->shift = shift;
    if (shift <= tol_abs) state->converged = 1;
  }
}

bool km_sizes_ok(long long N, int K) { return N >= 1 && N < (1ll << 31) && K >= 1 && K <= KM_MAXK; }
// the workspace of skf_kmeans_step_f32: sums and counts (zeroed every step: all in front of the partials), a partial per tile; -> its size
size_t km_carve(void* ws, long long N, int K, KmParams& p) {
  SkfWsCarver c(ws);
  p.sums = c.take<u64>(2 * (size_t)K); p.counts = c.take<unsigned>(K); p.partials = c.take<double>(skf_cdiv((long)N, KM_TILE));
  return c.used;
}
size_t km_smem_bytes(int K, bool acc) {
  const size_t Kp = ((size_t)K + 1) & ~(size_t)1;
  return Kp * 8 + (acc ? (size_t)K * 16 + 32 + (size_t)K * 4 : 0);
}
static_assert(((size_t)KM_MAXK * 8 + (size_t)KM_MAXK * 20 + 32) <= 160 * 1024, "LDS budget of one CU");

// the argument checks both entry points share; messages carry the entry point's name
#define KM_CHECK(cond, msg)                                        \
  do {                                                             \
    if (!(cond)) {                                                 \
      skf_set_error("%s: %s (%s)", fn, msg, #cond);                \
      return SKF_EINVAL;                                           \
    }                                                              \
  } while (0)
int km_check(const char* fn, const float* points, int ldp, long long N, int d, const float* centers, int ldc, int K) {
  if (d != 2) { skf_set_error("%s: only d == 2 is built (got d = %d)", fn, d); return SKF_EUNSUPPORTED; }
  KM_CHECK(K >= 1 && K <= KM_MAXK, "K must be in [1, 4096]");
  KM_CHECK(N >= 1 && N < (1ll << 31), "N must be in [1, 2^31)");
  KM_CHECK(points && centers, "null pointer");
  KM_CHECK(ldp >= 2 && ldc >= 2 && ldp % 2 == 0 && ldc % 2 == 0 && ((uintptr_t)points & 7) == 0 && ((uintptr_t)centers & 7) == 0,
           "rows must be 8-byte aligned (base pointers and row pitches)");
  return SKF_OK;
}

template <bool ACC>
int km_launch_assign(const KmParams& p, hipStream_t st) {
  const size_t smem = km_smem_bytes(p.K, ACC);
  if (smem > 64 * 1024) {
    static SkfOncePerDevice attr;
    if (attr.needed()) {
      SKF_HIP(hipFuncSetAttribute((const void*)kmeans_assign_kernel<ACC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)km_smem_bytes(KM_MAXK, ACC)));
      attr.mark();
    }
  }
  const int grid = p.ntiles < KM_MAXGRID ? p.ntiles : KM_MAXGRID;
  SkfProfScope ps_(st, ACC ? "kmeans_assign_accumulate<2048>" : "kmeans_assign<2048>", 6.0 * p.N * p.K, 8.0 * p.N + 4.0 * p.N);
  hipLaunchKernelGGL(kmeans_assign_kernel<ACC>, dim3(grid), dim3(KM_THREADS), smem, st, p);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

}  // namespace

extern "C" size_t skf_kmeans_workspace_bytes(long long N, int K) {
  if (!km_sizes_ok(N, K)) return 0;
  KmParams p;
  return km_carve(nullptr, N, K, p);
}

extern "C" int skf_kmeans_assign_f32(const float* points, int ldp, long long N, int d, const float* centers, int ldc, int K,
                                     int* labels, float* dist, skf_stream_t stream) {
  const int rc = km_check(__func__, points, ldp, N, d, centers, ldc, K);
  if (rc != SKF_OK) return rc;
  SKF_CHECK_ARG(labels, "null pointer");
  KmParams p{};
  p.pts = points; p.ctr = centers; p.labels = labels; p.dist = dist;
  p.N = (long)N; p.ldp = ldp; p.ldc = ldc; p.K = K; p.ntiles = skf_cdiv((long)N, KM_TILE); p.scale = 0.f;
  return km_launch_assign<false>(p, (hipStream_t)stream);
}

extern "C" int skf_kmeans_step_f32(const float* points, int ldp, long long N, int d, float* centers, int ldc, int K, int scale_exp,
                                   double tol_abs, int* labels, int* counts, SkfKmeansState* state, void* workspace,
                                   size_t workspace_bytes, skf_stream_t stream) {
  const int rc = km_check(__func__, points, ldp, N, d, centers, ldc, K);
  if (rc != SKF_OK) return rc;
  SKF_CHECK_ARG(labels && state && workspace, "null pointer");
  SKF_CHECK_ARG(scale_exp >= -126 && scale_exp <= 127, "scale_exp must be in [-126, 127]");
  SKF_CHECK_ARG(((uintptr_t)state & 7) == 0, "state must be 8-byte aligned");
  SKF_CHECK_ARG(workspace_bytes >= skf_kmeans_workspace_bytes(N, K) && ((uintptr_t)workspace & 15) == 0, "workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  KmParams p{};
  p.pts = points; p.ctr = centers; p.labels = labels; p.dist = nullptr; p.state = state;
  km_carve(workspace, N, K, p);
  p.N = (long)N; p.ldp = ldp; p.ldc = ldc; p.K = K; p.ntiles = skf_cdiv((long)N, KM_TILE);
  p.scale = __builtin_ldexpf(1.f, scale_exp);
  // the same three commands every iteration, converged or not (a stopped fit's kernels return at once; the zeroed accumulators are
  // then never read)
  SKF_HIP(hipMemsetAsync(workspace, 0, (size_t)((char*)p.partials - (char*)workspace), st));
  const int rc2 = km_launch_assign<true>(p, st);
  if (rc2 != SKF_OK) return rc2;
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(1), dim3(KM_THREADS), 0, st, centers, ldc, K, p.sums, p.counts, p.partials, p.ntiles,
                     (double)__builtin_ldexp(1.0, -scale_exp), tol_abs, counts, state);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
