// Exact O(N^2) t-SNE (van der Maaten & Hinton 2008, scikit-learn's method='exact') for the embedding map of the evaluation
// (include/skf.h: skf_tsne_affinities_f32, skf_tsne_step_f32, skf_tsne_kl_f32).  DESIGN.md section 3k.
//
//   tsne_dist_kernel     D_ij = sum_k (x_ik - x_jk)^2, fp32, k ascending, written into the P buffer (64 x 64 tiles, 4 x 4 per thread)
//   tsne_search_kernel   one workgroup per row: the row of D in LDS, 64 bisection steps of beta in fp64 -> beta_i, S_i, min_i
//   tsne_joint_kernel    in place over the P buffer: D_ij -> (float)((p_j|i + p_i|j) / 2N); needs D_ij alone because D_ij == D_ji
//   tsne_pair_kernel     one wave per row: Y in LDS once per workgroup, the P row in 16-byte loads -> z_i, a_i, r_i
//   tsne_update_kernel   Z in fp64 (every workgroup, the same order), gradient, gains / velocity / position update
//   tsne_klrow_kernel    one wave per row -> z_i (fp32), sum_j P log(P / q) and sum_j P (fp64);  tsne_klsum_kernel: one workgroup
//
// Determinism.  No floating-point atomic anywhere.  Every sum has one order that depends on N alone: a lane (thread) walks its
// elements in ascending index, the lanes of a wave meet in an xor butterfly, the waves of a workgroup are added in wave order.  A row
// belongs to one wave (or workgroup) wherever it runs, so the grid size does not enter.
#include "skf_common.h"

namespace {

constexpr int TS_MAXN = 8192;
constexpr int TS_MAXD = 1024;
constexpr int TS_STEPS = 64;                      // bisection steps, no early exit
constexpr int TS_THREADS = 256;                   // search, joint, update, klsum
constexpr int TS_PAIR_THREADS = 512;              // pair pass: 8 waves = 8 rows in flight per workgroup
constexpr int TS_PAIR_WAVES = TS_PAIR_THREADS / 64;
constexpr int TS_PAIR_MAXGRID = 512;              // 2 resident workgroups per CU at N = 8192 (64 KB of LDS each)
constexpr int TS_TILE = 64, TS_KC = 32;           // distance tiles

bool ts_n_ok(long long N) { return N >= 3 && N <= TS_MAXN; }

// ---------------------------------------------------------------- affinities
__global__ __launch_bounds__(256) void tsne_dist_kernel(const float* __restrict__ x, int ldx, int N, int d, float* __restrict__ D, int ldp) {
  __shared__ __align__(16) float sA[TS_KC][TS_TILE];       // [k][row]: a thread reads its 4 rows as one 16-byte word
  __shared__ __align__(16) float sB[TS_KC][TS_TILE];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * TS_TILE, j0 = blockIdx.x * TS_TILE;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < d; k0 += TS_KC) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = (tid >> 3) + 32 * h, k4 = (tid & 7) * 4;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;   // rows past N and columns past d read as 0: they add (0 - 0)^2
      if (k0 + k4 < d) {
        if (i0 + row < N) va = *(const float4*)(x + (size_t)(i0 + row) * ldx + k0 + k4);
        if (j0 + row < N) vb = *(const float4*)(x + (size_t)(j0 + row) * ldx + k0 + k4);
      }
      sA[k4][row] = va.x; sA[k4 + 1][row] = va.y; sA[k4 + 2][row] = va.z; sA[k4 + 3][row] = va.w;
      sB[k4][row] = vb.x; sB[k4 + 1][row] = vb.y; sB[k4 + 2][row] = vb.z; sB[k4 + 3][row] = vb.w;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < TS_KC; ++k) {              // k ascending: the order of the definition
      const float4 a = *(const float4*)&sA[k][ty * 4];
      const float4 b = *(const float4*)&sB[k][tx * 4];
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float df = av[r] - bv[c];
          acc[r][c] = fmaf(df, df, acc[r][c]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ty * 4 + r;
    if (i >= N) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + tx * 4 + c;
      if (j < N) D[(size_t)i * ldp + j] = acc[r][c];
    }
  }
}

// f(x) = (1 + x) log(1 + x) - x >= 0: its series below |x| = 1e-3, 1 at x <= -1 (the limit)
__device__ __forceinline__ double ts_f(double x) {
  if (fabs(x) < 1e-3) return x * x * (0.5 + x * (-1.0 / 6.0 + x * (1.0 / 12.0 + x * (-1.0 / 20.0 + x * (1.0 / 30.0)))));
  const double o = 1.0 + x;
  return o > 0.0 ? o * log1p(x) - x : -x;
}

__global__ __launch_bounds__(TS_THREADS) void tsne_search_kernel(const float* __restrict__ D, int ldp, int N, double log_perp,
                                                                 double log_n_over_perp, double* __restrict__ beta_out,
                                                                 double* __restrict__ s_out, float* __restrict__ min_out) {
  extern __shared__ __align__(16) float ts_row[];          // N floats: D_ij, or -1 for the entries the loop skips
  __shared__ double sRed[4], sRed2[4];
  __shared__ float sMin[4];
  __shared__ int sCnt[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* row = D + (size_t)i * ldp;
  // A distance of exactly zero (a duplicate of row i) has e = 0, p = 1 at every beta: such entries are COUNTED, not summed, so that
  // two identical rows - whose rows of D differ only in where the diagonal and the mutual zero sit - run the same additions.
  float mn = __builtin_inff();
  int nz = 0;
  for (int j = tid; j < N; j += TS_THREADS) {
    float v = row[j];
    if (j == i) v = -1.f;
    else {
      mn = fminf(mn, v);
      if (v == 0.f) { nz += 1; v = -1.f; }
    }
    ts_row[j] = v;
  }
  mn = -wave_max(-mn);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
  if ((tid & 63) == 0) { sMin[tid >> 6] = mn; sCnt[tid >> 6] = nz; }
  __syncthreads();
  const double m = (double)fminf(fminf(sMin[0], sMin[1]), fminf(sMin[2], sMin[3]));
  const double zeros = (double)(sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3]);
  const double n = (double)(N - 1);

  // scikit-learn's _binary_search_perplexity with the tolerance exit removed; every thread carries the same state
  double beta = 1.0, lo = 0.0, hi = __builtin_inf(), beta_used = 1.0, s_used = 1.0;
  for (int step = 0; step < TS_STEPS; ++step) {
    double s = 0.0, t = 0.0;
    for (int j = tid; j < N; j += TS_THREADS) {
      const float v = ts_row[j];
      if (v > 0.f) {
        const double e = (double)v - m;
        const double p = exp(-beta * e);
        s += p;
        t += e * p;
      }
    }
    s = block_sum(s, sRed) + zeros;
    t = block_sum(t, sRed2);
    double diff;                                   // H - log(perplexity), in the form that is well conditioned where the row stands
    if (s > 0.75 * n) {
      // near uniform: H - log n = -(1/n) sum_j f(n w_j - 1), n w_j - 1 = (expm1(-beta e_j) - mean) / (1 + mean); no cancellation
      double ms = 0.0;
      for (int j = tid; j < N; j += TS_THREADS) {
        const float v = ts_row[j];
        if (v > 0.f) ms += expm1(-beta * ((double)v - m));
      }
      const double mean = block_sum(ms, sRed) / n, onem = 1.0 + mean;
      double fs = 0.0;
      for (int j = tid; j < N; j += TS_THREADS) {
        const float v = ts_row[j];
        if (v > 0.f) fs += ts_f((expm1(-beta * ((double)v - m)) - mean) / onem);
      }
      fs = block_sum(fs, sRed2) + zeros * ts_f((0.0 - mean) / onem);
      diff = log_n_over_perp - fs / n;
    } else {
      diff = log(s) + beta * t / s - log_perp;
    }
    beta_used = beta; s_used = s;
    if (diff > 0.0) {
      lo = beta;
      beta = (hi == __builtin_inf()) ? beta * 2.0 : (beta + hi) * 0.5;
    } else {
      hi = beta;
      beta = (beta + lo) * 0.5;
    }
  }
  if (tid == 0) { beta_out[i] = beta_used; s_out[i] = s_used; min_out[i] = (float)m; }
}

__device__ __forceinline__ double ts_conditional(float dij, double beta, double m, double s) {
  return exp(-beta * ((double)dij - m)) / s;
}

__global__ __launch_bounds__(TS_THREADS) void tsne_joint_kernel(float* __restrict__ P, int ldp, int N, const double* __restrict__ beta,
                                                                const double* __restrict__ S, const float* __restrict__ mins) {
  const int i = blockIdx.y;
  const int j = blockIdx.x * TS_THREADS + threadIdx.x;
  if (j >= N) return;
  float* e = P + (size_t)i * ldp + j;
  if (j == i) { *e = 0.f; return; }
  const float dij = *e;                              // == D_ji bit for bit
  const double a = ts_conditional(dij, beta[i], (double)mins[i], S[i]);
  const double b = ts_conditional(dij, beta[j], (double)mins[j], S[j]);
  *e = (float)((a + b) / (2.0 * (double)N));         // a + b == b + a: entry (j, i) gets the same bits
}

// ---------------------------------------------------------------- gradient step
// lane-level walk of one row: f(j, P_ij, yj) for every j < N, j = 4 (lane + 64 t) + c; the P row in 16-byte loads, except the last
// N % 4 entries of a row, which are read one by one (nothing past column N - 1 is touched)
template <typename F>
__device__ __forceinline__ void ts_walk_row(const float* __restrict__ prow, const float2* __restrict__ sY, int N, int lane, F&& f) {
  for (int j4 = lane * 4; j4 < N; j4 += 256) {
    float pv[4] = {0.f, 0.f, 0.f, 0.f};
    if (j4 + 3 < N) {
      const float4 p = *(const float4*)(prow + j4);
      pv[0] = p.x; pv[1] = p.y; pv[2] = p.z; pv[3] = p.w;
    } else {
      for (int c = 0; j4 + c < N; ++c) pv[c] = prow[j4 + c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j4 + c;
      if (j < N) f(j, pv[c], sY[j]);
    }
  }
}

__device__ __forceinline__ void ts_stage_y(const float* __restrict__ Y, int N, float2* sY) {
  for (int j = threadIdx.x; j < N; j += blockDim.x) sY[j] = *(const float2*)(Y + 2 * (size_t)j);
  __syncthreads();
}

// q_ij is DEFINED as: dx = yi.x - yj.x; dy = yi.y - yj.y; v_rcp_f32(1 + fmaf(dy, dy, dx * dx))  (1 ulp)
__device__ __forceinline__ float ts_q(float dx, float dy) { return __builtin_amdgcn_rcpf(1.0f + fmaf(dy, dy, dx * dx)); }

__global__ __launch_bounds__(TS_PAIR_THREADS) void tsne_pair_kernel(const float* __restrict__ P, int ldp, int N, const float* __restrict__ Y,
                                                                    float* __restrict__ zrow, float2* __restrict__ arow,
                                                                    float2* __restrict__ rrow) {
  extern __shared__ __align__(16) float2 ts_y[];
  ts_stage_y(Y, N, ts_y);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x * TS_PAIR_WAVES + wave; i < N; i += gridDim.x * TS_PAIR_WAVES) {
    const float2 yi = ts_y[i];
    float z = 0.f, ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f;
    ts_walk_row(P + (size_t)i * ldp, ts_y, N, lane, [&](int j, float p, float2 yj) {
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float q = ts_q(dx, dy);
      const float pq = p * q, qq = q * q;
      z += (j == i) ? 0.f : q;
      ax = fmaf(pq, dx, ax); ay = fmaf(pq, dy, ay);
      rx = fmaf(qq, dx, rx); ry = fmaf(qq, dy, ry);
    });
    z = wave_sum(z); ax = wave_sum(ax); ay = wave_sum(ay); rx = wave_sum(rx); ry = wave_sum(ry);
    if (lane == 0) { zrow[i] = z; arow[i] = make_float2(ax, ay); rrow[i] = make_float2(rx, ry); }
  }
}

// Z = sum_i z_i in fp64: thread t adds z_t, z_{t+256}, ...; butterfly; waves in order.  Every workgroup computes the same bits.
__device__ __forceinline__ double ts_total_z(const float* __restrict__ zrow, int N, double* sRed) {
  double z = 0.0;
  for (int i = threadIdx.x; i < N; i += TS_THREADS) z += (double)zrow[i];
  return block_sum(z, sRed);
}

__global__ __launch_bounds__(TS_THREADS) void tsne_update_kernel(int N, const float* __restrict__ zrow, const float* __restrict__ arow,
                                                                 const float* __restrict__ rrow, float* __restrict__ Y,
                                                                 float* __restrict__ U, float* __restrict__ gains, float* __restrict__ grad,
                                                                 float exaggeration, float momentum, float lr) {
#pragma clang fp contract(off)
  __shared__ double sRed[4];
  const double Z = ts_total_z(zrow, N, sRed);
  const int e = blockIdx.x * TS_THREADS + threadIdx.x;       // element of the (N, 2) arrays
  if (e >= 2 * N) return;
  const float g = (float)(4.0 * ((double)exaggeration * (double)arow[e] - (double)rrow[e] / Z));
  if (grad) grad[e] = g;
  const float u = U[e], gn = gains[e];
  // one rounding per operation (contraction is off in this kernel)
  const float ug = u * g;
  float gn2 = (ug < 0.0f) ? gn + 0.2f : gn * 0.8f;
  gn2 = fmaxf(gn2, 0.01f);
  const float t1 = momentum * u;
  const float t2 = gn2 * g;
  const float t3 = lr * t2;
  const float u2 = t1 - t3;
  const float y2 = Y[e] + u2;
  gains[e] = gn2; U[e] = u2; Y[e] = y2;
}

// ---------------------------------------------------------------- KL divergence
__global__ __launch_bounds__(TS_PAIR_THREADS) void tsne_klrow_kernel(const float* __restrict__ P, int ldp, int N, const float* __restrict__ Y,
                                                                     float* __restrict__ zrow, double* __restrict__ krow,
                                                                     double* __restrict__ prow_sum) {
  extern __shared__ __align__(16) float2 ts_y[];
  ts_stage_y(Y, N, ts_y);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x * TS_PAIR_WAVES + wave; i < N; i += gridDim.x * TS_PAIR_WAVES) {
    const float2 yi = ts_y[i];
    float z = 0.f;
    double k = 0.0, ps = 0.0;
    ts_walk_row(P + (size_t)i * ldp, ts_y, N, lane, [&](int j, float p, float2 yj) {
      const float q = ts_q(yi.x - yj.x, yi.y - yj.y);
      z += (j == i) ? 0.f : q;
      if (p > 0.f && j != i) {
        k += (double)p * log((double)p / (double)q);
        ps += (double)p;
      }
    });
    z = wave_sum(z); k = wave_sum(k); ps = wave_sum(ps);
    if (lane == 0) { zrow[i] = z; krow[i] = k; prow_sum[i] = ps; }
  }
}

// KL = sum_{P > 0} P log(P Z / q) = sum_i k_i + log Z * sum_i s_i
__global__ __launch_bounds__(TS_THREADS) void tsne_klsum_kernel(int N, const float* __restrict__ zrow, const double* __restrict__ krow,
                                                                const double* __restrict__ prow_sum, double* __restrict__ out) {
  __shared__ double sRed[4];
  const double Z = ts_total_z(zrow, N, sRed);
  double k = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < N; i += TS_THREADS) { k += krow[i]; s += prow_sum[i]; }
  k = block_sum(k, sRed);
  s = block_sum(s, sRed);
  if (threadIdx.x == 0) *out = k + log(Z) * s;
}

// ---------------------------------------------------------------- host
struct TsWs { char* a; char* b; char* c; size_t total; };          // three arrays of 8 N bytes
TsWs ts_carve(void* ws, int N) {
  SkfWsCarver k(ws);
  TsWs w{k.take<char>((size_t)N * 8), k.take<char>((size_t)N * 8), k.take<char>((size_t)N * 8), 0};     // (braces: in this order)
  w.total = k.used;
  return w;
}

int ts_pair_grid(int N) {
  const int g = skf_cdiv(N, TS_PAIR_WAVES);
  return g < TS_PAIR_MAXGRID ? g : TS_PAIR_MAXGRID;
}

#define TS_CHECK_WS()                                                                                                             \
  SKF_CHECK_ARG(workspace && workspace_bytes >= skf_tsne_workspace_bytes(N) && ((uintptr_t)workspace & 15) == 0,                  \
                "workspace too small or misaligned")
#define TS_CHECK_P()                                                                                                              \
  SKF_CHECK_ARG(P && ldp >= N && ldp % 4 == 0 && ((uintptr_t)P & 15) == 0, "P rows must be 16-byte aligned (base pointer, ldp % 4 == 0, ldp >= N)")
#define TS_CHECK_N2(ptr, name)                                                                                                    \
  SKF_CHECK_ARG(ptr && ((uintptr_t)ptr & 7) == 0, name " must be a contiguous (N, 2) array, 8-byte aligned")

}  // namespace

extern "C" size_t skf_tsne_workspace_bytes(int N) {
  if (!ts_n_ok(N)) return 0;
  return ts_carve(nullptr, N).total;
}

extern "C" int skf_tsne_affinities_f32(const float* x, int ldx, int N, int d, double perplexity, float* P, int ldp, double* beta,
                                       void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_CHECK_ARG(ts_n_ok(N), "N must be in [3, 8192]");
  SKF_CHECK_ARG(d >= 4 && d <= TS_MAXD && d % 4 == 0, "d must be a multiple of 4 in [4, 1024]");
  SKF_CHECK_ARG(x && ldx >= d && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0, "x rows must be 16-byte aligned (base pointer, ldx % 4 == 0, ldx >= d)");
  TS_CHECK_P();
  SKF_CHECK_ARG(perplexity >= 1.0 && perplexity <= (double)(N - 1), "perplexity must be in [1, N - 1]");
  SKF_CHECK_ARG(!beta || ((uintptr_t)beta & 7) == 0, "beta must be 8-byte aligned");
  TS_CHECK_WS();
  hipStream_t st = (hipStream_t)stream;
  const TsWs w = ts_carve(workspace, N);
  double* bws = beta ? beta : (double*)w.a;
  const int nt = skf_cdiv(N, TS_TILE);
  {
    SkfProfScope ps_(st, "tsne_dist", 3.0 * N * N * d, 4.0 * N * N + 4.0 * N * d);
    hipLaunchKernelGGL(tsne_dist_kernel, dim3(nt, nt), dim3(256), 0, st, x, ldx, N, d, P, ldp);
    SKF_LAUNCH_CHECK();
  }
  SkfProfScope ps_(st, "tsne_search_joint", 0.0, 12.0 * N * N);
  hipLaunchKernelGGL(tsne_search_kernel, dim3(N), dim3(TS_THREADS), (size_t)N * 4, st, (const float*)P, ldp, N, log(perplexity), log((double)(N - 1) / perplexity), bws,
                     (double*)w.b, (float*)w.c);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_joint_kernel, dim3(skf_cdiv(N, TS_THREADS), N), dim3(TS_THREADS), 0, st, P, ldp, N, (const double*)bws,
                     (const double*)w.b, (const float*)w.c);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_tsne_step_f32(const float* P, int ldp, int N, float* Y, float* U, float* gains, float* grad, float exaggeration,
                                 float momentum, float learning_rate, void* workspace, size_t workspace_bytes, skf_stream_t stream) {
  SKF_CHECK_ARG(ts_n_ok(N), "N must be in [3, 8192]");
  TS_CHECK_P();
  TS_CHECK_N2(Y, "Y"); TS_CHECK_N2(U, "U"); TS_CHECK_N2(gains, "gains");
  SKF_CHECK_ARG(!grad || ((uintptr_t)grad & 7) == 0, "grad must be 8-byte aligned");
  TS_CHECK_WS();
  hipStream_t st = (hipStream_t)stream;
  const TsWs w = ts_carve(workspace, N);
  {
    SkfProfScope ps_(st, "tsne_pair", 14.0 * N * N, 4.0 * N * N);
    hipLaunchKernelGGL(tsne_pair_kernel, dim3(ts_pair_grid(N)), dim3(TS_PAIR_THREADS), (size_t)N * 8, st, P, ldp, N, (const float*)Y,
                       (float*)w.a, (float2*)w.b, (float2*)w.c);
    SKF_LAUNCH_CHECK();
  }
  SkfProfScope ps_(st, "tsne_update", 0.0, 40.0 * N);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(skf_cdiv(2 * N, TS_THREADS)), dim3(TS_THREADS), 0, st, N, (const float*)w.a,
                     (const float*)w.b, (const float*)w.c, Y, U, gains, grad, exaggeration, momentum, learning_rate);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_tsne_kl_f32(const float* P, int ldp, int N, const float* Y, double* kl_out, void* workspace, size_t workspace_bytes,
                               skf_stream_t stream) {
  SKF_CHECK_ARG(ts_n_ok(N), "N must be in [3, 8192]");
  TS_CHECK_P();
  TS_CHECK_N2(Y, "Y");
  SKF_CHECK_ARG(kl_out && ((uintptr_t)kl_out & 7) == 0, "kl_out must be an 8-byte aligned device double");
  TS_CHECK_WS();
  hipStream_t st = (hipStream_t)stream;
  const TsWs w = ts_carve(workspace, N);
  hipLaunchKernelGGL(tsne_klrow_kernel, dim3(ts_pair_grid(N)), dim3(TS_PAIR_THREADS), (size_t)N * 8, st, P, ldp, N, Y, (float*)w.a,
                     (double*)w.b, (double*)w.c);
  SKF_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_klsum_kernel, dim3(1), dim3(TS_THREADS), 0, st, N, (const float*)w.a, (const double*)w.b, (const double*)w.c,
                     kl_out);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
