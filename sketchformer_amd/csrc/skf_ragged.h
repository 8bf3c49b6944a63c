// What the kernels over ragged batches share (skf_tokenize.hip, skf_augment.hip, skf_simplify.hip): the data is `flat`, P rows, and
// `offsets`, N + 1 int64, item s owning the rows [offsets[s], offsets[s + 1]).  Only comparisons, min/max and integer work live
// here: nothing that a file's floating-point contraction setting could change.  The counts -> offsets scan is skf_ragged.hip
// (skf_common.h: skf_counts_to_offsets_launch).
#pragma once
#include "skf_common.h"

constexpr float SKF_SKETCH_LIMIT = 1000.0f;

// the loaders' clip of a raw value to +-1000 (the *_CLAMP flags)
__device__ __forceinline__ float skf_sketch_clamp(float v, int clamp) {
  return clamp ? fminf(fmaxf(v, -SKF_SKETCH_LIMIT), SKF_SKETCH_LIMIT) : v;
}

// The rows [beg, beg + n) that item s owns, cut to [0, P] whatever the offsets hold: this clamp alone keeps the kernels inside
// flat (and inside the per-row workspaces) on offsets that are negative, descending or past the end.
__device__ __forceinline__ void skf_ragged_range(const long long* offsets, long long s, long long P, long long& beg, int& n) {
  const long long a0 = offsets[s], a1 = offsets[s + 1];
  beg = a0 < 0 ? 0 : (a0 > P ? P : a0);
  const long long end = a1 < beg ? beg : (a1 > P ? P : a1);
  n = (int)(end - beg);                                                        // P < 2^31
}

// The argument checks of an entry point over (flat, P, offsets, N, workspace); a macro, so that the text names the entry point
// (SKF_CHECK_ARG's __func__) and its own parameter names.  `need` = what its *_workspace_bytes returns for these sizes.
#define SKF_RAGGED_CHECK_ARGS(flat, P, offsets, N, workspace, workspace_bytes, need)                                    \
  SKF_CHECK_ARG(flat && offsets && workspace, "null pointer");                                                         \
  SKF_CHECK_ARG(N >= 1, #N " must be at least 1");                                                                     \
  SKF_CHECK_ARG(P >= 1 && P < (1ll << 31), "P must be in [1, 2^31)");                                                  \
  SKF_CHECK_ARG(((uintptr_t)flat & 3) == 0 && ((uintptr_t)offsets & 7) == 0 && ((uintptr_t)workspace & 15) == 0,       \
                #flat " and " #offsets " must be aligned to their element, the workspace to 16 bytes");                \
  SKF_CHECK_ARG(workspace_bytes >= need, "workspace too small")
