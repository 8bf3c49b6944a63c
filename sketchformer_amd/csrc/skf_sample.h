// Sampled token selection of the decoder (include/skf.h: "the selection rule"): temperature, top-k cut, nucleus (top-p) cut and an
// inverse-CDF draw in index order, for ONE row of logits held in LDS, by one workgroup of SKF_SAMPLE_NT threads.  Used by
// decode_position_kernel (skf_decode_fused.hip: the row is the `hs` area) and by the stand-alone launch (skf_decode.hip).
//
// Everything after z = logit / temperature and e = exp(z - max z) is integer arithmetic:
//  - a value z is handled as its order-preserving 32-bit key, so both cuts are thresholds on the key (ties share one fate by
//    construction) and are found by a radix select: 4 passes of 8 bits over a 256-bin LDS histogram, no sort;
//  - a mass e is the integer floor(e * 2^32) (the maximum has mass 2^32, an entry more than 22.2 below it has mass 0), so every
//    histogram, sum and prefix sum is exact, does not depend on the order of its terms and needs no floating-point atomic: the
//    token is a pure function of (row, parameters, u).
// Temperature-only decoding (top_k = 0, top_p = 1) runs the max and the scan and neither radix select.
#pragma once
#include "skf_common.h"

constexpr int SKF_SAMPLE_NT = 512;                 // threads of the workgroup (8 waves)
constexpr int SKF_SAMPLE_SCRATCH_FLOATS = 640;     // LDS scratch skf_sample_row needs behind any 4-byte aligned pointer

typedef unsigned long long skf_u64;

// z_a < z_b <=> key_a < key_b; -0 and +0 share a key
__device__ __forceinline__ uint32_t skf_sample_key(float z) {
  uint32_t b = __float_as_uint(z);
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ skf_u64 skf_sample_mass(float z, float m) {
  return (skf_u64)(__expf(z - m) * 4294967296.0f);      // z <= m: at most 2^32
}
__device__ __forceinline__ skf_u64 skf_shfl_u64(skf_u64 v, int src_lane) {
  const uint32_t lo = __shfl((uint32_t)v, src_lane, 64), hi = __shfl((uint32_t)(v >> 32), src_lane, 64);
  return ((skf_u64)hi << 32) | lo;
}

// The key of the k-th largest value of zs[0..V) (1 <= k <= V).  hist: 256 words, bc: 2 words.  Ends with a barrier.
__device__ __forceinline__ uint32_t skf_sample_kth_key(const float* zs, int V, uint32_t k, uint32_t* hist, uint32_t* bc, int tid) {
  uint32_t prefix = 0, pmask = 0, need = k;          // the need-th largest of the keys that match prefix under pmask
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < V; j += SKF_SAMPLE_NT) {
      const uint32_t key = skf_sample_key(zs[j]);
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {                                  // lane = bins 4 lane .. 4 lane + 3; counts from the top bin down
      const uint32_t c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const uint32_t mine = c0 + c1 + c2 + c3;
      uint32_t suf = mine;                           // bins of this lane and of every higher lane
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_down(suf, o, 64);
        if (tid + o < 64) suf += t;
      }
      uint32_t a = suf - mine;                       // keys in higher bins
      if (a < need && suf >= need) {                 // exactly one lane holds the bin of the need-th largest
        int b = 3;
        if (a + c3 < need) { a += c3; b = 2; if (a + c2 < need) { a += c2; b = 1; if (a + c1 < need) { a += c1; b = 0; } } }
        bc[0] = 4 * tid + b; bc[1] = need - a;
      }
    }
    __syncthreads();
    prefix |= bc[0] << shift; pmask |= 255u << shift; need = bc[1];
  }
  return prefix;
}

// Nucleus threshold over the entries with key >= kmin (what top-k kept): with S their mass, the smallest key T such that the
// mass of kept entries with key > T is < top_p * S.  An entry survives iff key >= T: for such an entry the mass above it is at
// most the mass above T, and for any key below T the mass above it is >= top_p * S because T is the smallest.  The maximum
// always survives (nothing lies above it and top_p * S > 0).  hist: 256 64-bit words, bc: 2 words.  Ends with a barrier.
__device__ __forceinline__ uint32_t skf_sample_nucleus_key(const float* zs, int V, float m, uint32_t kmin, float top_p, skf_u64* hist,
                                                           skf_u64* bc, int tid) {
  uint32_t prefix = 0, pmask = 0;
  skf_u64 above = 0;                                 // mass of the kept entries above every key that matches the prefix
  double lim = 0.0;                                  // top_p * S (S < 2^49: exact in a double)
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < V; j += SKF_SAMPLE_NT) {
      const float z = zs[j];
      const uint32_t key = skf_sample_key(z);
      if (key >= kmin && (key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], skf_sample_mass(z, m));
    }
    __syncthreads();
    if (tid < 64) {
      const skf_u64 c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const skf_u64 mine = c0 + c1 + c2 + c3;
      skf_u64 suf = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const skf_u64 t = skf_shfl_u64(suf, (tid + o) & 63);
        if (tid + o < 64) suf += t;
      }
      if (shift == 24) lim = (double)top_p * (double)skf_shfl_u64(suf, 0);      // first pass: lane 0's suffix is S
      // the lowest bin whose mass above is < lim: this lane's top bin qualifies and the next lower lane's does not
      skf_u64 a = above + (suf - mine);
      if ((double)a < lim && (tid == 0 || !((double)(above + suf) < lim))) {
        int b = 3;
        if ((double)(a + c3) < lim) { a += c3; b = 2; if ((double)(a + c2) < lim) { a += c2; b = 1; if ((double)(a + c1) < lim) { a += c1; b = 0; } } }
        bc[0] = (skf_u64)(4 * tid + b); bc[1] = a;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)bc[0] << shift; pmask |= 255u << shift; above = bc[1];      // (lim lives in wave 0, its only reader)
  }
  return prefix;
}

// The token of one row.  zs[0..V): the logits, complete and visible to the workgroup (a barrier lies behind their last write);
// they are overwritten by z = logit / temperature.  bits24: the uniform u = bits24 * 2^-24.  scratch: SKF_SAMPLE_SCRATCH_FLOATS
// floats of LDS nobody else uses during the call, nor before the workgroup's next barrier after it (the token is read back from
// there).  Every thread of the workgroup calls it and every thread gets the token.
// The row's maximum must be finite: then it has mass 2^32, S > 0 and both selects find their bin.  A row whose maximum is not
// (every entry -inf or NaN, or a +inf) has no mass and gets V - 1 without running the cuts; NaN entries of other rows carry none.
__device__ __forceinline__ int skf_sample_row(float* zs, int V, float temperature, int top_k, float top_p, uint32_t bits24, float* scratch,
                                              int tid) {
  skf_u64* sp = reinterpret_cast<skf_u64*>(scratch + ((reinterpret_cast<uintptr_t>(scratch) >> 2) & 1));      // 8-byte aligned
  skf_u64* hist = sp;                                 // [256] bins of a radix pass
  skf_u64* wtot = sp + 256;                           // [8]   per-wave mass of the scan
  skf_u64* bc = sp + 264;                             // [2]   what wave 0 tells the workgroup
  int* tok = reinterpret_cast<int*>(sp + 266);        // [1]
  float* wmx = reinterpret_cast<float*>(sp + 267);    // [8]   per-wave maximum
  const int lane = tid & 63, wave = tid >> 6;
  // 1. z and its maximum
  float m = -INFINITY;
  for (int j = tid; j < V; j += SKF_SAMPLE_NT) {
    const float z = zs[j] / temperature;
    zs[j] = z;
    m = fmaxf(m, z);
  }
  m = wave_max(m);
  if (lane == 0) wmx[wave] = m;
  if (tid == 0) *tok = V - 1;                         // only a row without any mass keeps it
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SKF_SAMPLE_NT / 64; ++w) m = fmaxf(m, wmx[w]);
  if (!(fabsf(m) < INFINITY)) return V - 1;           // no finite maximum (all -inf / NaN, or a +inf): no mass to draw from
  // 2. 3. the cuts: survivors = keys >= kmin
  uint32_t kmin = 0;
  if (top_k > 0 && top_k < V)
    kmin = skf_sample_kth_key(zs, V, (uint32_t)top_k, reinterpret_cast<uint32_t*>(hist), reinterpret_cast<uint32_t*>(bc), tid);
  if (top_p < 1.0f) {
    const uint32_t kp = skf_sample_nucleus_key(zs, V, m, kmin, top_p, hist, bc, tid);
    kmin = kp > kmin ? kp : kmin;
  }
  // 4. inverse CDF in index order: thread t owns the entries [t c, (t + 1) c)
  const int c = (V + SKF_SAMPLE_NT - 1) / SKF_SAMPLE_NT;
  const int j0 = tid * c < V ? tid * c : V, j1 = j0 + c < V ? j0 + c : V;
  skf_u64 loc = 0;
  for (int j = j0; j < j1; ++j) {
    const float z = zs[j];
    if (skf_sample_key(z) >= kmin) loc += skf_sample_mass(z, m);
  }
  skf_u64 inc = loc;                                  // inclusive prefix over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const skf_u64 t = skf_shfl_u64(inc, (lane - o) & 63);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  skf_u64 total = 0;
#pragma unroll
  for (int w = 0; w < SKF_SAMPLE_NT / 64; ++w) {
    const skf_u64 t = wtot[w];
    if (w < wave) inc += t;
    total += t;
  }
  // r = floor(u * total) = (bits24 * total) >> 24 < total
  const skf_u64 r = (__umul64hi(total, (skf_u64)bits24) << 40) | ((total * (skf_u64)bits24) >> 24);
  skf_u64 acc = inc - loc;                            // exclusive prefix of this thread's entries
  if (acc <= r && r < inc) {                          // one thread: the prefix sum passes r among its entries
    for (int j = j0; j < j1; ++j) {
      const float z = zs[j];
      if (skf_sample_key(z) >= kmin) {
        acc += skf_sample_mass(z, m);
        if (acc > r) { *tok = j; break; }
      }
    }
  }
  __syncthreads();
  return *tok;
}
