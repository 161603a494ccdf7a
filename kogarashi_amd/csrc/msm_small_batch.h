// msm_small_batch.h -- the host-only, pure parts of the batched short MSM (kg_commit_batch, msm_small_batch.hip): the scratch one vector
// of a batch needs, how many vectors one launch group carries, where the groups begin, and the argument checks.  No HIP, no context:
// tests/host/msm_batch_host.cpp includes this file alone.
//
// Layout: vector b of a batch reads the n scalars at elements [b * stride, b * stride + n) of the caller's array (stride >= n, in elements
// of 4 words; the elements between two vectors are not read) and meets the ONE base array of the call.  A launch group is one launch of the
// short kernel's body with the vector in the grid's z dimension (msm_small_kernels.h: k_msm_small), one of the combine body for split
// windows (vector in y), and one of the finish kernel; between them a vector owns
//   [vector][W] window sums, 4 coordinates of 4 (G2: 8) u64 words each, ABI form -- what the single call leaves in its pinned host slot
//   [vector][W][NB][MSM_BATCH_PLANES] plane points of split windows (NB > 1), raw internal form, 36 (G2: 72) u32 words each
// of the context's grow-only batch scratch.  Groups run one after another on the stream over the same scratch.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include "curve_layout.h"

namespace kg {

// The limits of a launch group, named here and nowhere else:
constexpr size_t MSM_BATCH_GRID_MAX = 65535;                    // a HIP grid's y and z dimensions carry at most 65535 blocks
constexpr size_t MSM_BATCH_SCRATCH_CAP = (size_t)64 << 20;      // scratch of one group: at most 64 MiB -- a memory policy: a quarter of what
                                                                // the batched transform allows itself (ntt_batch.h), the inputs here are short
constexpr int MSM_BATCH_PLANES = 8;                             // plane points a workgroup of a split window leaves (= SM_MAX_R + 1, asserted in msm_small_batch.hip)

// The shape the short kernel runs an n-pair vector in (msm_small_plan / msm_small_glv): window width c, 2^r buckets per workgroup,
// halved scalars or not.  n == 0 is the shape without windows: the finish kernel alone writes the identities.
struct MsmBatchShape { int curve, c, r; bool glv; size_t n; };
inline int msm_batch_windows(const MsmBatchShape& s) { return s.n == 0 ? 0 : ((s.glv ? 128 : 255) + s.c - 1) / s.c; }
inline int msm_batch_ranges(const MsmBatchShape& s) { return s.n == 0 ? 1 : 1 << (s.c - 1 - s.r); }          // NB: workgroups per window
inline size_t msm_batch_sums_bytes(const MsmBatchShape& s) { return (size_t)msm_batch_windows(s) * xyzz_words64(s.curve) * 8; }
inline size_t msm_batch_planes_bytes(const MsmBatchShape& s) {
  const int NB = msm_batch_ranges(s);
  return NB > 1 ? (size_t)msm_batch_windows(s) * NB * MSM_BATCH_PLANES * raw_xyzz_words32(s.curve) * 4 : 0;
}
inline size_t msm_batch_vector_bytes(const MsmBatchShape& s) { return msm_batch_sums_bytes(s) + msm_batch_planes_bytes(s); }

// the most vectors one launch group carries: min(65535, cap / scratch bytes per vector), at least one
inline size_t msm_batch_per_launch(size_t vector_bytes) {
  if (vector_bytes == 0) return MSM_BATCH_GRID_MAX;
  const size_t by_scratch = MSM_BATCH_SCRATCH_CAP / vector_bytes;
  if (by_scratch < 1) return 1;
  return by_scratch < MSM_BATCH_GRID_MAX ? by_scratch : MSM_BATCH_GRID_MAX;
}
// number of groups a batch of `count` is cut into (0: count == 0 or per_launch == 0)
inline size_t msm_batch_groups(size_t per_launch, size_t count) { return per_launch == 0 || count == 0 ? 0 : (count - 1) / per_launch + 1; }
// group g of the batch: vectors [first, first + count)
struct MsmBatchGroup { size_t first, count; };
inline MsmBatchGroup msm_batch_group(size_t per_launch, size_t count, size_t g) {
  const size_t first = g * per_launch;
  return {first, count - first < per_launch ? count - first : per_launch};
}
// scratch bytes a batch of `count` needs: one group's worth
inline size_t msm_batch_scratch_bytes(size_t vector_bytes, size_t count) {
  const size_t per = msm_batch_per_launch(vector_bytes);
  return (count < per ? count : per) * vector_bytes;
}

// The argument checks of kg_commit_batch (true = acceptable), made before anything is dereferenced.  count == 0 is acceptable with any
// array pointers (nothing is enqueued); the outputs are needed whenever a point is written (n == 0 writes identities), bases and scalars
// whenever a pair is read.  Every element count and byte size the call forms must fit a size_t.
inline bool msm_batch_args_ok(const void* ctx, int curve, const void* d_bases, const void* d_scalars, size_t n, size_t count, size_t stride, const void* d_out_xy,
                              const void* d_out_inf) {
  if (!ctx || !curve_ok(curve) || stride < n) return false;
  if (count == 0) return true;
  if (!d_out_xy || !d_out_inf) return false;
  if (n != 0 && (!d_bases || !d_scalars)) return false;
  if (stride > SIZE_MAX / 32 / count) return false;                               // count * stride scalars of 32 bytes
  if (count > SIZE_MAX / (8 * affine_words64(curve))) return false;               // count points of 2 coordinates
  if (n > SIZE_MAX / (8 * affine_words64(curve))) return false;                   // n bases
  return true;
}

}  // namespace kg
