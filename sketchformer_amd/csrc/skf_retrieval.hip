// Exact k-nearest-neighbour search over embeddings (include/skf.h: skf_knn_topk_f32) and the row-normalising pre-pass of the
// cosine metric.  DESIGN.md section 3f.
//
// Three launches, no allocation:
//   knn_norms_kernel    ||q||^2 and ||g||^2, one wave per row, a fixed summation order (a row's norm does not depend on where it sits)
//   knn_partial_kernel  a workgroup owns 64 queries and one contiguous range of the gallery; it streams 128-row gallery tiles,
//                       forms the 128 x 64 dot products on v_mfma_f32_32x32x2_f32 (bit-for-bit a k-ordered fmaf chain per
//                       (gallery row, query) pair: the same pair gives the same bits wherever the row sits and however the
//                       gallery is split), and keeps every query's candidates in LDS.  The scores never leave the registers.
//   knn_merge_kernel    one wave per query merges the sorted partial lists of the gallery ranges.
//
// A candidate is ONE 64-bit key: (order-preserving image of the fp32 distance) << 32 | gallery index.  Unsigned order of the keys
// is (distance, index) order, so "ties resolve to the lower index" and "the result does not depend on the split" both follow
// from the keys being totally ordered: every stage selects the k smallest keys of a set, whatever order they arrived in.
#include "skf_common.h"

namespace {

typedef unsigned long long u64;
constexpr u64 KNN_MAXKEY = ~0ull;
constexpr int KNN_BQ = 64;        // queries per workgroup
constexpr int KNN_BG = 128;       // gallery rows per tile (4 waves x 32)
constexpr int KNN_DK = 32;        // contraction depth of one staged chunk
constexpr int KNN_CAP = 256;      // candidate slots per query (k <= 128 leaves >= one whole tile of free slots after a compaction)
constexpr int KNN_MAXK = 128;
constexpr int KNN_MAXS = 64;      // gallery ranges per query (one lane of the merging wave each)
constexpr int KNN_THREADS = 256;

constexpr int KNN_OFF_A = KNN_BQ * KNN_CAP * 8;                  // candidate keys first
constexpr int KNN_OFF_B = KNN_OFF_A + KNN_BG * KNN_DK * 4;
constexpr int KNN_OFF_THR = KNN_OFF_B + KNN_BQ * KNN_DK * 4;
constexpr int KNN_OFF_GN = KNN_OFF_THR + KNN_BQ * 8;
constexpr int KNN_OFF_THRF = KNN_OFF_GN + KNN_BG * 4;
constexpr int KNN_OFF_CNT = KNN_OFF_THRF + KNN_BQ * 4;
constexpr int KNN_OFF_FLAG = KNN_OFF_CNT + KNN_BQ * 4;
constexpr int KNN_SMEM = KNN_OFF_FLAG + 16;                      // 157,200 B: one workgroup per CU
static_assert(KNN_SMEM <= 160 * 1024, "LDS budget of one CU");

__device__ __forceinline__ unsigned knn_ord(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float knn_unord(unsigned o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ u64 knn_min(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 knn_max(u64 a, u64 b) { return a < b ? b : a; }

// Ascending bitonic sort of 256 keys held by one wave, key e = j * 64 + lane in v[j].
__device__ __forceinline__ void knn_sort256(u64 (&v)[4], int lane) {
#pragma unroll
  for (int size = 2; size <= 256; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
      if (stride >= 64) {
        const int js = stride >> 6;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if ((j & js) == 0) {
            const bool asc = ((j * 64) & size) == 0;      // bits 6, 7 of e are j's
            const u64 lo = knn_min(v[j], v[j | js]), hi = knn_max(v[j], v[j | js]);
            v[j] = asc ? lo : hi;
            v[j | js] = asc ? hi : lo;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u64 other = __shfl_xor(v[j], stride, 64);
          const bool lower = (lane & stride) == 0;
          const bool asc = ((j * 64 + lane) & size) == 0;
          v[j] = (lower == asc) ? knn_min(v[j], other) : knn_max(v[j], other);
        }
      }
    }
  }
}

struct KnnParams {
  const float* q; const float* g; const float* qn; const float* gn; const int* excl; u64* part;
  int ldq, ldg, Q, G, d, k, S, rows_per_split, nqt;
};

// One wave: keep the k smallest of query qq's candidates (sorted, in v and in LDS), refresh its count and threshold.
__device__ __forceinline__ void knn_compact(u64* sBuf, u64* sThr, float* sThrF, int* sCnt, int qq, int k, int lane, u64 (&v)[4]) {
  u64* buf = sBuf + qq * KNN_CAP;
  const int n = min(sCnt[qq], KNN_CAP);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (j * 64 + lane < n) ? buf[j * 64 + lane] : KNN_MAXKEY;
  knn_sort256(v, lane);
#pragma unroll
  for (int j = 0; j < 2; ++j) buf[j * 64 + lane] = v[j];          // k <= 128: the survivors are in v[0], v[1]
  const u64 t0 = __shfl(v[0], (k - 1) & 63, 64), t1 = __shfl(v[1], (k - 1) & 63, 64);
  const u64 thr = (k - 1) >= 64 ? t1 : t0;                         // MAXKEY while fewer than k candidates were seen
  if (lane == 0) {
    sCnt[qq] = min(n, k);
    sThr[qq] = thr;
    sThrF[qq] = thr == KNN_MAXKEY ? __builtin_inff() : knn_unord((unsigned)(thr >> 32));
  }
}

__global__ __launch_bounds__(KNN_THREADS) void knn_partial_kernel(KnnParams p) {
  extern __shared__ __align__(16) unsigned char knn_smem[];
  u64* sBuf = (u64*)knn_smem;
  float4* sA4 = (float4*)(knn_smem + KNN_OFF_A);
  float4* sB4 = (float4*)(knn_smem + KNN_OFF_B);
  u64* sThr = (u64*)(knn_smem + KNN_OFF_THR);
  float* sGn = (float*)(knn_smem + KNN_OFF_GN);
  float* sThrF = (float*)(knn_smem + KNN_OFF_THRF);
  int* sCnt = (int*)(knn_smem + KNN_OFF_CNT);
  int* sFlag = (int*)(knn_smem + KNN_OFF_FLAG);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  // query tile fastest: the workgroups that run together stream the same gallery range (L2)
  const int s = blockIdx.x / p.nqt, qt = blockIdx.x - s * p.nqt;
  const int q0 = qt * KNN_BQ;
  const int gBeg = s * p.rows_per_split, gEnd = min(p.G, gBeg + p.rows_per_split);
  const int nchunks = (p.d + KNN_DK - 1) / KNN_DK;

  if (tid < KNN_BQ) {
    const bool valid = q0 + tid < p.Q;
    sThr[tid] = valid ? KNN_MAXKEY : 0ull;                         // rows behind Q accept nothing
    sThrF[tid] = valid ? __builtin_inff() : -__builtin_inff();
    sCnt[tid] = 0;
  }
  if (tid == 0) *sFlag = 0;

  float qn[2]; int excl[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int qi = q0 + 32 * a + r;
    qn[a] = qi < p.Q ? p.qn[qi] : 0.f;
    excl[a] = (p.excl && qi < p.Q) ? p.excl[qi] : -1;
  }

  // staging: thread t moves 16-byte piece cc of rows rr + 32 i (8 lanes = one 128-byte row segment)
  const int cc = tid & 7, rr = tid >> 3;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[4], rb[2];
  auto load = [&](int g0, int c) {
    const int kk = c * KNN_DK + cc * 4;
    const bool kin = kk < p.d;                                      // d % 4 == 0: a piece is inside or outside as a whole
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = g0 + rr + 32 * i;
      ra[i] = (kin && row < gEnd) ? *(const float4*)(p.g + (size_t)row * p.ldg + kk) : zero4;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = q0 + rr + 32 * i;
      rb[i] = (kin && row < p.Q) ? *(const float4*)(p.q + (size_t)row * p.ldq + kk) : zero4;
    }
  };
  // LDS image: 128-byte rows, piece index XOR (row >> 1) & 7 (16 consecutive rows of one piece column fall on 16 different slots)
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int row = rr + 32 * i; sA4[row * 8 + (cc ^ ((row >> 1) & 7))] = ra[i]; }
#pragma unroll
    for (int i = 0; i < 2; ++i) { const int row = rr + 32 * i; sB4[row * 8 + (cc ^ ((row >> 1) & 7))] = rb[i]; }
  };

  const int arow = 32 * w + r;                                      // this lane's gallery row of the tile (A operand)
  const int aswz = (arow >> 1) & 7, bswz = (r >> 1) & 7;            // (32 + r) >> 1 & 7 == (r >> 1) & 7

  if (gBeg < gEnd) load(gBeg, 0);
  for (int g0 = gBeg; g0 < gEnd; g0 += KNN_BG) {
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;

    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();                                              // the previous chunk's fragments are read
      store();
      if (c == 0 && tid < KNN_BG) sGn[tid] = (g0 + tid < gEnd) ? p.gn[g0 + tid] : __builtin_inff();
      __syncthreads();
      if (c + 1 < nchunks) load(g0, c + 1);
      else if (g0 + KNN_BG < gEnd) load(g0 + KNN_BG, 0);
      // lane (r, h) supplies contraction index 8 jj + 4 h + i of its row to MFMA i of group jj, on both operands alike
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float4 av = sA4[arow * 8 + ((2 * jj + h) ^ aswz)];
        const float4 b0 = sB4[r * 8 + ((2 * jj + h) ^ bswz)];
        const float4 b1 = sB4[(32 + r) * 8 + ((2 * jj + h) ^ bswz)];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b0.z, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b1.z, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b0.w, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b1.w, acc[1], 0, 0, 0);
      }
    }

    // ---- the tile's scores: acc[a][e] = g[row] . q[32 a + r], row = 32 w + (e & 3) + 8 (e >> 2) + 4 h
    float gnr[16];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 t = *(const float4*)&sGn[32 * w + 8 * m + 4 * h];
      gnr[4 * m] = t.x; gnr[4 * m + 1] = t.y; gnr[4 * m + 2] = t.z; gnr[4 * m + 3] = t.w;
    }
    unsigned pend = 0;                                              // bit 16 a + e: that score still has to be offered
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float tf = sThrF[32 * a + r];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        acc[a][e] = fmaf(-2.f, acc[a][e], qn[a] + gnr[e]);         // the squared distance, from here on
        if (acc[a][e] <= tf) pend |= 1u << (16 * a + e);
      }
    }
    for (;;) {
      if (pend) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const unsigned bit = 1u << (16 * a + e);
            if (pend & bit) {
              const int ql = 32 * a + r;
              const int idx = g0 + 32 * w + (e & 3) + 8 * (e >> 2) + 4 * h;
              const u64 key = ((u64)knn_ord(acc[a][e]) << 32) | (unsigned)idx;
              bool keep = false;
              if (idx < gEnd && idx != excl[a] && key < sThr[ql]) {
                const int slot = atomicAdd(&sCnt[ql], 1);
                if (slot < KNN_CAP) sBuf[ql * KNN_CAP + slot] = key;
                else { *sFlag = 1; keep = true; }                   // full: offered again after the compaction
              }
              if (!keep) pend &= ~bit;
            }
          }
        }
      }
      __syncthreads();
      if (*sFlag == 0) break;
      __syncthreads();                                              // everybody has seen the flag
      if (tid == 0) *sFlag = 0;
      for (int qq = 16 * w; qq < 16 * w + 16; ++qq) {
        if (sCnt[qq] >= KNN_CAP) { u64 v[4]; knn_compact(sBuf, sThr, sThrF, sCnt, qq, p.k, lane, v); }
      }
      __syncthreads();
    }
  }

  __syncthreads();
  for (int qq = 16 * w; qq < 16 * w + 16; ++qq) {
    if (q0 + qq >= p.Q) break;
    u64 v[4];
    knn_compact(sBuf, sThr, sThrF, sCnt, qq, p.k, lane, v);
    u64* out = p.part + ((size_t)(q0 + qq) * p.S + s) * p.k;
    if (lane < p.k) out[lane] = v[0];
    if (64 + lane < p.k) out[64 + lane] = v[1];
  }
}

__device__ __forceinline__ u64 knn_wave_min(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = knn_min(v, __shfl_xor(v, o, 64));
  return v;
}

// One wave per query: S sorted lists of k keys -> the k smallest, as (index, distance).
__global__ __launch_bounds__(KNN_THREADS) void knn_merge_kernel(const u64* part, int Q, int S, int k, int* out_idx, float* out_dist) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6);
  if (q >= Q) return;
  const u64* lists = part + (size_t)q * S * k;
  if (S == 1) {
    for (int e = lane; e < k; e += 64) {
      const u64 m = lists[e];
      out_idx[(size_t)q * k + e] = m == KNN_MAXKEY ? -1 : (int)(unsigned)m;
      out_dist[(size_t)q * k + e] = knn_unord((unsigned)(m >> 32));
    }
    return;
  }
  const u64* mine = lists + (size_t)min(lane, S - 1) * k;
  int pos = 0;
  u64 head = lane < S ? mine[0] : KNN_MAXKEY;
  for (int i = 0; i < k; ++i) {
    const u64 m = knn_wave_min(head);
    if (lane == 0) {
      out_idx[(size_t)q * k + i] = m == KNN_MAXKEY ? -1 : (int)(unsigned)m;
      out_dist[(size_t)q * k + i] = knn_unord((unsigned)(m >> 32));
    }
    if (head == m && m != KNN_MAXKEY) {                             // keys are unique: exactly one lane advances
      ++pos;
      head = pos < k ? mine[pos] : KNN_MAXKEY;
    }
  }
}

// ||x||^2 of rows [0, Qrows) of a and [0, Grows) of b into na / nb: one wave per row, lane l sums columns 4 l + 256 i in order,
// then the xor butterfly - the same order for every row.
__device__ __forceinline__ float knn_row_sumsq(const float* x, int d, int lane) {
  float s = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *(const float4*)(x + c);
    s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
  }
  return wave_sum(s);
}
__global__ __launch_bounds__(KNN_THREADS) void knn_norms_kernel(const float* a, int lda, int Qrows, const float* b, int ldb, int Grows,
                                                                int d, float* na, float* nb) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= (long)Qrows + Grows) return;
  const bool isq = row < Qrows;
  const long rl = isq ? row : row - Qrows;
  const float s = knn_row_sumsq(isq ? a + (size_t)rl * lda : b + (size_t)rl * ldb, d, lane);
  if (lane == 0) (isq ? na : nb)[rl] = s;
}
__global__ __launch_bounds__(KNN_THREADS) void row_normalize_kernel(const float* x, int ldx, int rows, int d, float* y, int ldy) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * ldx;
  float* yr = y + (size_t)row * ldy;
  const float n = fmaxf(sqrtf(knn_row_sumsq(xr, d, lane)), 1e-12f);
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *(const float4*)(xr + c);
    *(float4*)(yr + c) = make_float4(v.x / n, v.y / n, v.z / n, v.w / n);
  }
}

// How the gallery is cut: whole 128-row tiles per range, enough ranges that few queries still fill the chip, never more than
// one lane of the merging wave per range, and at least 8 tiles per range (every range ends with a sort per query).
struct KnnSplit { int S, rows_per_split, nqt; };
KnnSplit knn_split(int Q, int G) {
  KnnSplit r;
  r.nqt = skf_cdiv(Q, KNN_BQ);
  const int nt = skf_cdiv(G, KNN_BG);
  int want = skf_cdiv(768, r.nqt);
  want = want < KNN_MAXS ? want : KNN_MAXS;
  const int most = nt / 8 > 1 ? nt / 8 : 1;
  want = want < most ? want : most;
  const int per = skf_cdiv(nt, want);
  r.rows_per_split = per * KNN_BG;
  r.S = skf_cdiv(G, r.rows_per_split);
  return r;
}
bool knn_sizes_ok(int Q, int G, int k) { return Q >= 1 && G >= 1 && k >= 1 && k <= KNN_MAXK && k <= G; }
// the workspace of skf_knn_topk_f32: query norms, gallery norms, then the partial lists, which end it without rounding; -> its size
size_t knn_carve(void* ws, int Q, int G, int k, int S, KnnParams& p) {
  SkfWsCarver c(ws);
  p.qn = c.take<float>(Q); p.gn = c.take<float>(G); p.part = c.take<u64>(0);
  return c.used + (size_t)Q * S * k * 8;
}

}  // namespace

extern "C" size_t skf_knn_workspace_bytes(int Q, int G, int k) {
  if (!knn_sizes_ok(Q, G, k)) return 0;
  const KnnSplit sp = knn_split(Q, G);
  KnnParams p;
  return knn_carve(nullptr, Q, G, k, sp.S, p);
}

extern "C" int skf_knn_topk_f32(const float* queries, int ldq, int Q, const float* gallery, int ldg, int G, int d, int k,
                                const int* exclude, int* out_idx, float* out_dist, void* workspace, size_t workspace_bytes,
                                skf_stream_t stream) {
  SKF_CHECK_ARG(queries && gallery && out_idx && out_dist && workspace, "null pointer");
  SKF_CHECK_ARG(Q >= 1 && G >= 1, "Q and G must be at least 1");
  SKF_CHECK_ARG(d >= 4 && d <= 1024 && d % 4 == 0, "d must be a multiple of 4 in [4, 1024]");
  SKF_CHECK_ARG(k >= 1 && k <= KNN_MAXK, "k must be in [1, 128]");
  SKF_CHECK_ARG(k <= (exclude ? G - 1 : G), "k exceeds the gallery rows a query can be given (G, or G - 1 with exclude)");
  SKF_CHECK_ARG(ldq >= d && ldg >= d && ldq % 4 == 0 && ldg % 4 == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)gallery & 15) == 0,
                "rows must be 16-byte aligned (base pointers and row pitches)");
  SKF_CHECK_ARG(workspace_bytes >= skf_knn_workspace_bytes(Q, G, k) && ((uintptr_t)workspace & 15) == 0, "workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  const KnnSplit sp = knn_split(Q, G);
  KnnParams p;
  p.q = queries; p.g = gallery; p.excl = exclude;
  knn_carve(workspace, Q, G, k, sp.S, p);
  p.ldq = ldq; p.ldg = ldg; p.Q = Q; p.G = G; p.d = d; p.k = k; p.S = sp.S; p.rows_per_split = sp.rows_per_split; p.nqt = sp.nqt;
  static SkfOncePerDevice attr;
  if (attr.needed()) {
    SKF_HIP(hipFuncSetAttribute((const void*)knn_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, KNN_SMEM));
    attr.mark();
  }
  const long nrows = (long)Q + G;
  hipLaunchKernelGGL(knn_norms_kernel, dim3(skf_cdiv(nrows, KNN_THREADS / 64)), dim3(KNN_THREADS), 0, st, queries, ldq, Q, gallery, ldg, G, d, (float*)p.qn, (float*)p.gn);
  SKF_LAUNCH_CHECK();
  {
    SkfProfScope ps_(st, "knn_partial<64x128,f32>", 2.0 * Q * G * d, 4.0 * ((double)sp.nqt * G * d + (double)Q * d) + 8.0 * Q * sp.S * k);
    hipLaunchKernelGGL(knn_partial_kernel, dim3(sp.nqt * sp.S), dim3(KNN_THREADS), KNN_SMEM, st, p);
    SKF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(knn_merge_kernel, dim3(skf_cdiv(Q, KNN_THREADS / 64)), dim3(KNN_THREADS), 0, st, p.part, Q, sp.S, k, out_idx, out_dist);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_row_normalize_f32(const float* x, int ldx, int rows, int d, float* y, int ldy, skf_stream_t stream) {
  SKF_CHECK_ARG(x && y, "null pointer");
  SKF_CHECK_ARG(rows >= 1, "rows must be at least 1");
  SKF_CHECK_ARG(d >= 4 && d <= 1024 && d % 4 == 0, "d must be a multiple of 4 in [4, 1024]");
  SKF_CHECK_ARG(ldx >= d && ldy >= d && ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0,
                "rows must be 16-byte aligned (base pointers and row pitches)");
  hipLaunchKernelGGL(row_normalize_kernel, dim3(skf_cdiv(rows, KNN_THREADS / 64)), dim3(KNN_THREADS), 0, (hipStream_t)stream, x, ldx, rows, d, y, ldy);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
