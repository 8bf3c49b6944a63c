// Sequence alignment on the device (include/skf.h: skf_edit_distance_i64, skf_dtw_f32): unit-cost Levenshtein distance over token
// ids and dynamic time warping over pen positions, one pair per wavefront.  The reference has nothing in their place; the
// specification is the host restatement of tests/align_reference.py, which both kernels match exactly (DTW: bit for bit).
// DESIGN.md section 3n.
//
// The sweep.  Both distances fill a (La, Lb) table whose cell depends on its upper, left and upper-left neighbours.  A wave sweeps
// it as a systolic array: lane l owns the strip of S consecutive columns l S .. l S + S - 1 of b, with its operands and the last
// row it computed in registers; at tick t it computes row t - l of its strip.  The left-edge value it needs was computed by lane
// l - 1 one tick earlier and arrives with one cross-lane move per tick (DPP wave_shr:1, a v_mov_b32_dpp: no LDS round trip as a
// ds_bpermute would take); the value received the tick before is the diagonal.  A pair takes La + (lanes in use) - 1 ticks of S
// cells; there is no table in memory and no barrier inside the sweep.  Row a is read once into LDS (one barrier, before the
// sweep) and lane l reads element t - l from it, one tick ahead of its use: the addresses of a wave are consecutive, so the read
// has no bank conflict.
//
// Borders and limits.  The table's outer border is part of the recurrence (edit distance: D(i, -1) = i + 1, D(-1, j) = j + 1;
// DTW: +infinity with D(-1, -1) = 0, so that min() of the three neighbours returns the finite one exactly and the borders
// become running sums) and is the only place a constant enters a min().  Columns at and behind Lb are NOT padded with anything
// that must lose a min(): they are computed from zero operands like any other column, and since a cell only ever feeds cells to
// its right and below, nothing computed there can reach a column in front of Lb.  The answer is read from the lane and the
// register that hold column Lb - 1 (the per-lane column limit), wherever in a strip that is.
//
// Rounding (DTW).  Every cell is c + min(up, left, diag) with c = sqrt(dx * dx + dy * dy): four roundings and a correctly rounded
// square root (hipcc's default), no fused multiply-add: this file is compiled with -ffp-contract=off (build.SOURCE_FLAGS) and
// carries the pragma below as well.  min() is exact, so the value of a cell does not depend on the order of the sweep and a
// float32 numpy restatement row by row gives the same bits.
//
// Work split.  Paired mode: a workgroup of four waves takes four pairs, every wave with an LDS row of its own.  Cross mode: the
// four waves share ONE query row in LDS against four gallery rows, so a query row is read from memory once per four results.
// Registers and LDS as compiled: profiles/align_build.txt.
#include "skf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ALIGN_WAVES = 4;
constexpr int ALIGN_THREADS = ALIGN_WAVES * SKF_WAVE;

// dst[l] = src[l - 1] across the whole wave; lane 0 keeps `first`.  Must run with every lane of the wave enabled.
__device__ __forceinline__ int wave_shift_up(int src, int first) {
  return __builtin_amdgcn_update_dpp(first, src, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ float wave_shift_up(float src, float first) {
  return __builtin_bit_cast(float, wave_shift_up(__builtin_bit_cast(int, src), __builtin_bit_cast(int, first)));
}

// Levenshtein: D(i, j) = min(D(i-1, j) + 1, D(i, j-1) + 1, D(i-1, j-1) + (a_i != b_j)) = 1 + min(up, left, diag - (a_i == b_j)).
struct EditOp {
  typedef long long Elem;
  typedef int Val;
  typedef long long Raw;
  static __device__ __forceinline__ Elem load(const Raw* row, int idx, int n) { return idx < n ? row[idx] : 0ll; }
  static __device__ __forceinline__ int length(int n) { return n; }                          // an empty side stays empty
  static __device__ __forceinline__ Val top(int j) { return j; }                              // D(-1, j - 1): j cells to the left
  static __device__ __forceinline__ Val left(int i) { return i + 1; }                         // D(i, -1)
  static __device__ __forceinline__ Val cell(Elem a, Elem b, Val up, Val lf, Val dg) {
    return 1 + min(min(up, lf), dg - (a == b ? 1 : 0));
  }
};

// DTW: D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)), c = sqrt(dx dx + dy dy); outside the table +inf, D(-1, -1) = 0.
struct DtwOp {
  typedef float2 Elem;
  typedef float Val;
  typedef float Raw;
  static __device__ __forceinline__ Elem load(const Raw* row, int idx, int n) {
    return idx < n ? make_float2(row[2 * idx], row[2 * idx + 1]) : make_float2(0.0f, 0.0f);
  }
  static __device__ __forceinline__ int length(int n) { return n < 1 ? 1 : n; }              // empty: the single point (0, 0)
  static __device__ __forceinline__ Val top(int j) { return j == 0 ? 0.0f : __builtin_inff(); }
  static __device__ __forceinline__ Val left(int) { return __builtin_inff(); }
  static __device__ __forceinline__ Val cell(Elem a, Elem b, Val up, Val lf, Val dg) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    const float c = sqrtf(dx * dx + dy * dy);                        // correctly rounded: hipcc's default for sqrtf
    return c + fminf(fminf(up, lf), dg);
  }
};

template <class Op, int S, bool CROSS>
__global__ __launch_bounds__(ALIGN_THREADS) void align_kernel(const typename Op::Raw* __restrict__ a, long long lda,
                                                              const int* __restrict__ len_a, int Na, int Ta,
                                                              const typename Op::Raw* __restrict__ b, long long ldb,
                                                              const int* __restrict__ len_b, int Nb, int Tb, int groups,
                                                              typename Op::Val* __restrict__ out) {
  typedef typename Op::Elem Elem;
  typedef typename Op::Val Val;
  __shared__ Elem sA[CROSS ? 1 : ALIGN_WAVES][SKF_ALIGN_MAX_LEN];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform, and known to be
  // the pair of this wave
  long long ia, ib;
  if (CROSS) {
    ia = blockIdx.x / groups;
    ib = (long long)(blockIdx.x % groups) * ALIGN_WAVES + wave;
  } else {
    ia = ib = (long long)blockIdx.x * ALIGN_WAVES + wave;
  }
  const bool live = ia < Na && ib < Nb;                           // (a wave without a pair still meets the barrier below)
  const long long ra = ia < Na ? ia : Na - 1, rb = ib < Nb ? ib : Nb - 1;
  // (the lengths are the same in every lane of a wave; read as such, the loop below is counted in scalar registers)
  const int na = __builtin_amdgcn_readfirstlane(min(max(len_a[ra], 0), Ta)), nb = __builtin_amdgcn_readfirstlane(min(max(len_b[rb], 0), Tb));
  const int La = Op::length(na), Lb = Op::length(nb);

  // row a -> LDS: cross mode by the whole workgroup, paired mode by the wave that owns it
  {
    const typename Op::Raw* rowa = a + (size_t)ra * lda;
    Elem* dst = sA[CROSS ? 0 : wave];
    const int first = CROSS ? (int)threadIdx.x : lane, step = CROSS ? ALIGN_THREADS : SKF_WAVE;
    for (int i = first; i < La; i += step) dst[i] = Op::load(rowa, i, na);
  }
  // this lane's strip of b, in registers; columns at and behind Lb hold zeros and are never part of the answer
  Elem bs[S];
  {
    const typename Op::Raw* rowb = b + (size_t)rb * ldb;
#pragma unroll
    for (int s = 0; s < S; ++s) bs[s] = Op::load(rowb, lane * S + s, nb);
  }
  __syncthreads();
  if (!live) return;
  const size_t o = CROSS ? (size_t)ia * Nb + ib : (size_t)ia;
  if (La == 0 || Lb == 0) {                                       // (edit distance only) an empty side: the other side's length
    if (lane == 0) out[o] = (Val)(La + Lb);
    return;
  }

  const Elem* rowa = sA[CROSS ? 0 : wave];
  const int last_lane = (Lb - 1) / S;                             // the lane that holds column Lb - 1
  const int ticks = La + last_lane;
  Val prev[S];                                                    // the row above: D(i - 1, lane S + s)
#pragma unroll
  for (int s = 0; s < S; ++s) prev[s] = Op::top(lane * S + s + 1);
  Val diag = Op::top(lane * S);                                   // D(i - 1, lane S - 1)
  Val edge = prev[S - 1];                                         // this lane's last column of the row it computed last
  Elem a_next = rowa[0];                                          // lane 0's row 0; every other lane re-reads before its row 0
  for (int t = 0; t < ticks; ++t) {
    const int i = t - lane;
    const bool active = i >= 0 && i < La;
    const Elem a_cur = a_next;
    a_next = rowa[min(max(i + 1, 0), La - 1)];                    // next tick's element, in flight during this tick's cells
    const Val lf0 = wave_shift_up(edge, Op::left(t));             // lane 0 (i == t): the table's left border
    Val lf = lf0, dg = diag, cur[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      cur[s] = Op::cell(a_cur, bs[s], prev[s], lf, dg);
      dg = prev[s];
      lf = cur[s];
    }
    if (active) {
#pragma unroll
      for (int s = 0; s < S; ++s) prev[s] = cur[s];
      edge = cur[S - 1];
      diag = lf0;
    }
  }
  if (lane == last_lane) {
    const int col = (Lb - 1) - last_lane * S;
    Val r = prev[0];
#pragma unroll
    for (int s = 1; s < S; ++s) r = col == s ? prev[s] : r;
    out[o] = r;
  }
}

template <class Op>
int align_launch(const typename Op::Raw* a, long long lda, const int* len_a, int Na, int Ta, const typename Op::Raw* b, long long ldb,
                 const int* len_b, int Nb, int Tb, int cross, typename Op::Val* out, hipStream_t st) {
  const long long groups = (Nb + ALIGN_WAVES - 1) / ALIGN_WAVES;
  const long long blocks = cross ? (long long)Na * groups : groups;
  if (blocks >= (1ll << 31)) {
    skf_set_error("%s: Na * ceil(Nb / 4) must be below 2^31", __func__);
    return SKF_EINVAL;
  }
  const dim3 grid((unsigned)blocks), block(ALIGN_THREADS);
#define SKF_ALIGN_LAUNCH(S)                                                                                                     \
  do {                                                                                                                          \
    if (cross) hipLaunchKernelGGL((align_kernel<Op, S, true>), grid, block, 0, st, a, lda, len_a, Na, Ta, b, ldb, len_b, Nb, Tb, \
                                  (int)groups, out);                                                                            \
    else hipLaunchKernelGGL((align_kernel<Op, S, false>), grid, block, 0, st, a, lda, len_a, Na, Ta, b, ldb, len_b, Nb, Tb,      \
                            (int)groups, out);                                                                                  \
  } while (0)
  // the narrowest strip whose 64 lanes cover Tb columns
  if (Tb <= 64) SKF_ALIGN_LAUNCH(1);
  else if (Tb <= 128) SKF_ALIGN_LAUNCH(2);
  else if (Tb <= 256) SKF_ALIGN_LAUNCH(4);
  else SKF_ALIGN_LAUNCH(8);
#undef SKF_ALIGN_LAUNCH
  return SKF_OK;
}

}  // namespace

#define SKF_ALIGN_CHECK_SHAPES(width)                                                                                  \
  SKF_CHECK_ARG(len_a && len_b && out, "null pointer");                                                               \
  SKF_CHECK_ARG(Na >= 1 && Nb >= 1, "Na and Nb must be at least 1");                                                  \
  SKF_CHECK_ARG(Ta >= 1 && Tb >= 1, "Ta and Tb must be at least 1");                                                  \
  SKF_CHECK_ARG(Ta <= SKF_ALIGN_MAX_LEN && Tb <= SKF_ALIGN_MAX_LEN, "Ta and Tb must not exceed SKF_ALIGN_MAX_LEN");   \
  SKF_CHECK_ARG(lda >= (long long)(width) * Ta && ldb >= (long long)(width) * Tb, "a row stride is shorter than its row"); \
  SKF_CHECK_ARG(cross == 0 || cross == 1, "cross must be 0 or 1");                                                    \
  SKF_CHECK_ARG(cross || Na == Nb, "paired mode needs Na == Nb");                                                     \
  SKF_CHECK_ARG(((uintptr_t)len_a & 3) == 0 && ((uintptr_t)len_b & 3) == 0 && ((uintptr_t)out & 3) == 0,              \
                "the lengths and out must be 4-byte aligned")

extern "C" int skf_edit_distance_i64(const long long* a, long long lda, const int* len_a, int Na, int Ta, const long long* b,
                                     long long ldb, const int* len_b, int Nb, int Tb, int cross, int* out, skf_stream_t stream) {
  SKF_CHECK_ARG(a && b, "null pointer");
  SKF_ALIGN_CHECK_SHAPES(1);
  SKF_CHECK_ARG(((uintptr_t)a & 7) == 0 && ((uintptr_t)b & 7) == 0, "a and b must be 8-byte aligned");
  const int rc = align_launch<EditOp>(a, lda, len_a, Na, Ta, b, ldb, len_b, Nb, Tb, cross, out, (hipStream_t)stream);
  if (rc != SKF_OK) return rc;
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}

extern "C" int skf_dtw_f32(const float* xy_a, long long lda, const int* n_a, int Na, int Ta, const float* xy_b, long long ldb,
                           const int* n_b, int Nb, int Tb, int cross, float* out, skf_stream_t stream) {
  const int *len_a = n_a, *len_b = n_b;
  SKF_CHECK_ARG(xy_a && xy_b, "null pointer");
  SKF_ALIGN_CHECK_SHAPES(2);
  SKF_CHECK_ARG(((uintptr_t)xy_a & 3) == 0 && ((uintptr_t)xy_b & 3) == 0, "xy_a and xy_b must be 4-byte aligned");
  const int rc = align_launch<DtwOp>(xy_a, lda, len_a, Na, Ta, xy_b, ldb, len_b, Nb, Tb, cross, out, (hipStream_t)stream);
  if (rc != SKF_OK) return rc;
  SKF_LAUNCH_CHECK();
  return SKF_OK;
}
