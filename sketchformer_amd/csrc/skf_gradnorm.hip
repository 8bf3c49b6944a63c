// Gradient norms, clip scales and the skip decision over a flat fp32 buffer described by SkfParamEntry rows
// (tf.keras optimizers' clipnorm / global_clipnorm, tf.clip_by_norm / tf.clip_by_global_norm; the skip rule is
// LossScaleOptimizer's "a step with a non-finite gradient is not an optimizer iteration").
//
// The segment plan cuts every entry into chunks of kSegChunk LOGICAL elements (row-major over the entry's rows x cols view; the last
// chunk of an entry is ragged).  The chunk size is a constant of the library, not a function of the device: a result depends on the
// entry table alone, never on the grid size or the CU count.  Launch 1 gives every chunk one workgroup of 256 threads; a thread
// squares its elements into four fp64 accumulators (lane c of the 16-byte loads, the scalar tail into lane 0), folds them
// ((a0 + a1) + a2) + a3, the wave folds by the xor butterfly, the four waves fold in order 0..3 (block_sum of skf_common.h) - one
// fp64 partial and one count of non-finite elements per chunk, no atomics.  Launch 2 (one workgroup) folds an entry's partials in
// chunk order and the entries in table order, takes the square roots and writes norms, scales and the skip decision.
//
// The gaps between entries (the layout pads every entry to 4 floats) belong to no chunk and are never read; the fused wq|wk|wv
// blocks are read as the strided views their entries describe.
//
// Built with -ffp-contract=off (build.py): the scale c / max(norm, c) and the in-place x * s_e are single rounded operations that
// the float32 restatement of tests/clip_reference.py repeats bit for bit.
#include <math.h>
#include <string.h>
#include <vector>
#include "skf_common.h"

#define SKF_TRY_RC(call)               \
  do {                                 \
    int rc__ = (call);                 \
    if (rc__ != SKF_OK) return rc__;   \
  } while (0)

namespace {

constexpr int kSegChunk = SKF_SEGMENT_CHUNK;      // logical elements per chunk: 64 per thread, 16 16-byte loads
static_assert(kSegChunk % 1024 == 0, "a chunk is a whole number of 16-byte loads per thread");

// one chunk of work: logical elements [begin, begin + count) of entry `entry`
struct SegChunk {
  int64_t offset;       // the entry's first float in the flat buffer
  int32_t cols;         // logical columns (a contiguous entry is planned as one row of rows * cols)
  int32_t row_stride;   // floats between rows
  int32_t begin, count;
  int32_t entry;
  int32_t vec;          // 1: every 4 logical elements from `begin` on are one aligned 16-byte word (offset, cols, row_stride % 4 == 0)
};
// per entry: its chunks are [first, first + n)
struct SegEntry { int32_t first, n; };
struct SegHeader { int32_t n_entries, n_chunks, chunk_elems, pad; };
static_assert(sizeof(SegChunk) == 32 && sizeof(SegEntry) == 8 && sizeof(SegHeader) == 16, "plan layout");

__host__ __device__ inline const SegEntry* plan_entries(const void* plan) {
  return reinterpret_cast<const SegEntry*>(static_cast<const char*>(plan) + sizeof(SegHeader));
}
__host__ __device__ inline const SegChunk* plan_chunks(const void* plan, int n_entries) {
  // (the entry table is padded to a multiple of 16 bytes: the chunks start on a 16-byte boundary of the plan)
  const size_t ent = ((size_t)n_entries * sizeof(SegEntry) + 15) & ~(size_t)15;
  return reinterpret_cast<const SegChunk*>(static_cast<const char*>(plan) + sizeof(SegHeader) + ent);
}
size_t plan_bytes(int n_entries, int n_chunks) {
  const size_t ent = ((size_t)n_entries * sizeof(SegEntry) + 15) & ~(size_t)15;
  return sizeof(SegHeader) + ent + (size_t)n_chunks * sizeof(SegChunk);
}

// float index (relative to the entry's offset) of logical element e
__device__ __forceinline__ size_t seg_addr(const SegChunk& c, int e) {
  if (c.row_stride == c.cols) return (size_t)e;
  const int r = e / c.cols;
  return (size_t)r * (size_t)c.row_stride + (size_t)(e - r * c.cols);
}

__device__ __forceinline__ void seg_acc(float x, double& a, unsigned& bad) {
  a += (double)x * (double)x;
  bad += !(fabsf(x) <= 3.402823466e+38f);      // inf and NaN
}

__global__ __launch_bounds__(256) void seg_sumsq_kernel(const float* __restrict__ flat, const void* __restrict__ plan, int n_entries,
                                                        double* __restrict__ part, unsigned* __restrict__ part_bad) {
  __shared__ double sRed[4];
  const SegChunk c = plan_chunks(plan, n_entries)[blockIdx.x];
  const float* base = flat + c.offset;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  unsigned bad = 0;
  const int nq = c.vec ? (c.count >> 2) : 0;
  // four 16-byte loads in flight per thread, accumulated in the order q, q + 256, ..: a load past the end contributes +0.0 and no
  // count, so the sums are those of the plain loop over q
  for (int q0 = threadIdx.x; q0 < nq; q0 += 4 * 256) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + 256 * u;
      v[u] = q < nq ? *reinterpret_cast<const float4*>(base + seg_addr(c, c.begin + 4 * q)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { seg_acc(v[u].x, a0, bad); seg_acc(v[u].y, a1, bad); seg_acc(v[u].z, a2, bad); seg_acc(v[u].w, a3, bad); }
  }
  for (int i = (nq << 2) + threadIdx.x; i < c.count; i += 256) seg_acc(base[seg_addr(c, c.begin + i)], a0, bad);
  const double sum = block_sum(((a0 + a1) + a2) + a3, sRed);
  const double nbad = block_sum((double)bad, sRed);      // (integers below 2^53: exact in any order)
  if (threadIdx.x == 0) { part[blockIdx.x] = sum; part_bad[blockIdx.x] = (unsigned)nbad; }
}

// stats words (include/skf.h): [0] global norm, [1] applied global scale, [2] non-finite count (u32), [3] skip flag (u32),
// [4] skipped total (u32, only the sweeps add to it), [5..7] reserved, then E norms, then E scales
__global__ __launch_bounds__(256) void seg_finish_kernel(const void* __restrict__ plan, int n_entries, const double* __restrict__ part,
                                                         const unsigned* __restrict__ part_bad, double* __restrict__ entry_ss,
                                                         float grad_scale, int mode, float threshold, int skip_nonfinite,
                                                         float* __restrict__ stats) {
  __shared__ double sRed[4];
  const SegEntry* ent = plan_entries(plan);
  unsigned my_bad = 0;
  for (int e = threadIdx.x; e < n_entries; e += 256) {
    double ss = 0.0;
    for (int k = 0; k < ent[e].n; ++k) { ss += part[ent[e].first + k]; my_bad += part_bad[ent[e].first + k]; }
    entry_ss[e] = ss;
  }
  // (the counts are integers below 2^53: exact in any order.  block_sum's barriers also publish entry_ss to thread 0)
  const unsigned bad = (unsigned)block_sum((double)my_bad, sRed);
  __syncthreads();
  if (threadIdx.x == 0) {
    double ss = 0.0;
    for (int e = 0; e < n_entries; ++e) ss += entry_ss[e];
    const float norm = (float)(sqrt(ss) * (double)grad_scale);      // rounded once
    const float s = mode == SKF_CLIP_GLOBAL ? threshold / fmaxf(norm, threshold) : 1.0f;
    stats[0] = norm;
    stats[1] = s;
    reinterpret_cast<unsigned*>(stats)[2] = bad;
    reinterpret_cast<unsigned*>(stats)[3] = (skip_nonfinite && bad) ? 1u : 0u;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_entries; e += 256) {
    const float norm = (float)(sqrt(entry_ss[e]) * (double)grad_scale);
    stats[8 + e] = norm;
    stats[8 + n_entries + e] = mode == SKF_CLIP_PER_VARIABLE ? threshold / fmaxf(norm, threshold) : 1.0f;
  }
}

__global__ __launch_bounds__(256) void seg_scale_kernel(float* __restrict__ flat, const void* __restrict__ plan, int n_entries,
                                                        const float* __restrict__ scales, const unsigned* __restrict__ skip) {
  if (skip && *skip) return;
  const SegChunk c = plan_chunks(plan, n_entries)[blockIdx.x];
  float* base = flat + c.offset;
  const float s = scales[c.entry];
  const int nq = c.vec ? (c.count >> 2) : 0;
  for (int q0 = threadIdx.x; q0 < nq; q0 += 4 * 256) {      // four loads in flight, then the four stores (distinct words)
    float4* p[4];
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + 256 * u;
      p[u] = q < nq ? reinterpret_cast<float4*>(base + seg_addr(c, c.begin + 4 * q)) : nullptr;
      if (p[u]) v[u] = *p[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (p[u]) { v[u].x *= s; v[u].y *= s; v[u].z *= s; v[u].w *= s; *p[u] = v[u]; }
  }
  for (int i = (nq << 2) + threadIdx.x; i < c.count; i += 256) base[seg_addr(c, c.begin + i)] *= s;
}

// the checks every entry of a table must pass, and its chunk count
int entry_chunks(const SkfParamEntry& e, int i, long long* n_out) {
  if (e.offset < 0 || e.rows < 1 || e.cols < 1 || e.row_stride < e.cols) {
    skf_set_error("segment plan: entry %d has offset %lld, %d x %d, row stride %d (need offset >= 0, rows, cols >= 1, row_stride >= cols)",
                  i, (long long)e.offset, e.rows, e.cols, e.row_stride);
    return SKF_EINVAL;
  }
  const long long n = (long long)e.rows * e.cols;
  if (n >= (1ll << 31) - kSegChunk) { skf_set_error("segment plan: entry %d has %lld elements (limit 2^31 - %d)", i, n, kSegChunk); return SKF_EINVAL; }
  *n_out = n;
  return SKF_OK;
}

int check_plan_counts(const char* who, int n_entries, int n_chunks) {
  if (n_entries < 1 || n_chunks < n_entries) {
    skf_set_error("%s: %d entries in %d chunks (an entry has at least one chunk)", who, n_entries, n_chunks);
    return SKF_EINVAL;
  }
  return SKF_OK;
}

struct NormWs { double* part; double* entry_ss; unsigned* bad; size_t used; };
NormWs carve_norm_ws(void* ws, int n_entries, int n_chunks) {
  SkfWsCarver c(ws);
  NormWs w;
  w.part = c.take<double>((size_t)n_chunks);
  w.entry_ss = c.take<double>((size_t)n_entries);
  w.bad = c.take<unsigned>((size_t)n_chunks);
  w.used = c.used;
  return w;
}

}  // namespace

extern "C" int skf_segment_plan_chunks(const SkfParamEntry* entries_host, int n_entries) {
  SKF_CHECK_ARG(entries_host && n_entries >= 1, "no entries");
  long long chunks = 0;
  for (int i = 0; i < n_entries; ++i) {
    long long n = 0;
    int rc = entry_chunks(entries_host[i], i, &n);
    if (rc != SKF_OK) return rc;
    chunks += (n + kSegChunk - 1) / kSegChunk;
  }
  SKF_CHECK_ARG(chunks < (1ll << 31), "too many chunks");
  return (int)chunks;
}

extern "C" size_t skf_segment_plan_bytes(int n_entries, int n_chunks) {
  if (n_entries < 1 || n_chunks < n_entries) return 0;
  return plan_bytes(n_entries, n_chunks);
}

extern "C" int skf_segment_plan_build(const SkfParamEntry* entries_host, int n_entries, void* plan_host, size_t plan_bytes_given) {
  const int n_chunks = skf_segment_plan_chunks(entries_host, n_entries);
  if (n_chunks < 0) return n_chunks;
  SKF_CHECK_ARG(plan_host && plan_bytes_given >= plan_bytes(n_entries, n_chunks), "plan buffer too small (skf_segment_plan_bytes)");
  memset(plan_host, 0, plan_bytes(n_entries, n_chunks));
  SegHeader* h = static_cast<SegHeader*>(plan_host);
  h->n_entries = n_entries; h->n_chunks = n_chunks; h->chunk_elems = kSegChunk;
  SegEntry* ent = const_cast<SegEntry*>(plan_entries(plan_host));
  SegChunk* ch = const_cast<SegChunk*>(plan_chunks(plan_host, n_entries));
  int k = 0;
  for (int i = 0; i < n_entries; ++i) {
    const SkfParamEntry& e = entries_host[i];
    const long long n = (long long)e.rows * e.cols;
    const bool contiguous = e.rows == 1 || e.row_stride == e.cols;
    SegChunk c{};
    c.offset = e.offset; c.entry = i;
    c.cols = contiguous ? (int)n : e.cols;
    c.row_stride = contiguous ? (int)n : e.row_stride;
    c.vec = (e.offset & 3) == 0 && (contiguous || ((e.cols & 3) == 0 && (e.row_stride & 3) == 0));
    ent[i].first = k;
    for (long long b = 0; b < n; b += kSegChunk) {
      c.begin = (int)b;
      c.count = (int)(n - b < kSegChunk ? n - b : kSegChunk);
      ch[k++] = c;
    }
    ent[i].n = k - ent[i].first;
  }
  return SKF_OK;
}

extern "C" size_t skf_segment_norms_workspace_bytes(int n_entries, int n_chunks) {
  if (n_entries < 1 || n_chunks < n_entries) return 0;
  return carve_norm_ws(nullptr, n_entries, n_chunks).used;
}

extern "C" size_t skf_segment_stats_floats(int n_entries) { return n_entries < 1 ? 0 : 8 + 2 * (size_t)n_entries; }

extern "C" int skf_gradient_clip_validate(int mode, float threshold, float clipvalue) {
  SKF_CHECK_ARG(mode == SKF_CLIP_NONE || mode == SKF_CLIP_PER_VARIABLE || mode == SKF_CLIP_GLOBAL,
                "mode must be 0 (none), 1 (per variable: clipnorm) or 2 (global: global_clipnorm)");
  if (mode != SKF_CLIP_NONE && clipvalue != 0.0f) {
    skf_set_error("gradient clip: a norm mode and clipvalue are both set; at most one of clipnorm, global_clipnorm and clipvalue "
                  "may be given (Keras refuses the combination too)");
    return SKF_EINVAL;
  }
  if (mode != SKF_CLIP_NONE && !(threshold > 0.0f && threshold <= 3.402823466e+38f)) {
    skf_set_error("gradient clip: the norm threshold must be finite and > 0 (got %g)", (double)threshold);
    return SKF_EINVAL;
  }
  if (!(clipvalue >= 0.0f && clipvalue <= 3.402823466e+38f)) {
    skf_set_error("gradient clip: clipvalue must be finite and > 0, or 0 for off (got %g)", (double)clipvalue);
    return SKF_EINVAL;
  }
  return SKF_OK;
}

extern "C" int skf_segment_norms(const float* flat, const void* plan_dev, int n_entries, int n_chunks, float grad_scale, int mode,
                                 float threshold, int skip_nonfinite, void* workspace, size_t workspace_bytes, float* stats,
                                 skf_stream_t stream) {
  SKF_CHECK_ARG(flat && plan_dev && workspace && stats, "null operand");
  SKF_CHECK_ARG(((uintptr_t)flat & 15) == 0 && ((uintptr_t)plan_dev & 15) == 0 && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)stats & 3) == 0,
                "flat and plan must be 16-byte aligned, the workspace 256-byte aligned");
  SKF_TRY_RC(check_plan_counts(__func__, n_entries, n_chunks));
  SKF_TRY_RC(skf_gradient_clip_validate(mode, threshold, 0.0f));
  const NormWs w = carve_norm_ws(workspace, n_entries, n_chunks);
  SKF_CHECK_ARG(workspace_bytes >= w.used, "workspace too small (skf_segment_norms_workspace_bytes)");
  hipStream_t s = (hipStream_t)stream;
  {
    SkfProfScope ps(s, "grad_sumsq", 0.0, 0.0);
    hipLaunchKernelGGL(seg_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, flat, plan_dev, n_entries, w.part, w.bad);
    SKF_LAUNCH_CHECK();
  }
  SkfProfScope ps(s, "grad_norms", 0.0, 0.0);
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(256), 0, s, plan_dev, n_entries, (const double*)w.part, (const unsigned*)w.bad,
                     w.entry_ss, grad_scale, mode, threshold, skip_nonfinite, stats);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_segment_scale(float* flat, const void* plan_dev, int n_entries, int n_chunks, const float* scales,
                                 const void* skip, skf_stream_t stream) {
  SKF_CHECK_ARG(flat && plan_dev && scales, "null operand");
  SKF_CHECK_ARG(((uintptr_t)flat & 15) == 0 && ((uintptr_t)plan_dev & 15) == 0 && ((uintptr_t)scales & 3) == 0 && ((uintptr_t)skip & 3) == 0,
                "flat and plan must be 16-byte aligned");
  SKF_TRY_RC(check_plan_counts(__func__, n_entries, n_chunks));
  SkfProfScope ps((hipStream_t)stream, "grad_segment_scale", 0.0, 0.0);
  hipLaunchKernelGGL(seg_scale_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, flat, plan_dev, n_entries, scales,
                     (const unsigned*)skip);
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
