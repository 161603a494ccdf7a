// ntt_batch.h -- the host-only, pure parts of the batched transform (kg_ntt_bn254_fr_batch, ntt_batch.hip): how many transforms one
// launch group carries, where the groups begin, the element strides of every plan step and the argument checks.  No HIP, no context:
// tests/host/ntt_batch_plan_host.cpp includes this file alone.
//
// Layout: transform b of a batch occupies elements [b * stride, b * stride + n) of the caller's array (stride >= n = 2^log_n, in
// elements of 4 words); the elements between two transforms are neither read nor written.  A plan step (ntt_tile.h: ntt_plan) is one
// launch whose grid is (tiles of one transform, transforms of the group); a multi-step plan keeps transform b's intermediate values
// in scratch elements [b * n, b * n + n) of the context's grow-only NTT scratch.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

namespace kg {

// The two limits of a launch group, named here and nowhere else:
constexpr size_t NTT_BATCH_GRID_Y_MAX = 65535;        // a HIP grid's y dimension carries at most 65535 blocks
constexpr uint32_t NTT_BATCH_SCRATCH_LOG = 23;        // scratch of one group: at most 2^23 elements (256 MiB) -- a memory policy: twice
                                                      // what the benchmark's own 2^22 transform makes a context keep
constexpr uint32_t NTT_BATCH_ONE_STEP_MAX_LOG = 11;   // transforms up to this size are one step (= NTT_MAX_LOG_M, asserted in ntt_batch.hip): no scratch

inline bool ntt_batch_log_ok(uint32_t log_n) { return log_n >= 1 && log_n <= 28; }

// the most transforms of 2^log_n elements one launch group carries (0: log_n outside 1..28)
inline size_t ntt_batch_per_launch(uint32_t log_n) {
  if (!ntt_batch_log_ok(log_n)) return 0;
  if (log_n <= NTT_BATCH_ONE_STEP_MAX_LOG) return NTT_BATCH_GRID_Y_MAX;
  const size_t by_scratch = log_n >= NTT_BATCH_SCRATCH_LOG ? 1 : (size_t)1 << (NTT_BATCH_SCRATCH_LOG - log_n);
  return by_scratch < NTT_BATCH_GRID_Y_MAX ? by_scratch : NTT_BATCH_GRID_Y_MAX;
}
// number of groups a batch of `count` is cut into (0: log_n outside 1..28 or count == 0); groups run one after another on the stream
inline size_t ntt_batch_groups(uint32_t log_n, size_t count) {
  const size_t per = ntt_batch_per_launch(log_n);
  return per == 0 || count == 0 ? 0 : (count - 1) / per + 1;
}
// group g of the batch: transforms [first, first + count)
struct NttBatchGroup { size_t first, count; };
inline NttBatchGroup ntt_batch_group(size_t per_launch, size_t count, size_t g) {
  const size_t first = g * per_launch;
  return {first, count - first < per_launch ? count - first : per_launch};
}
// scratch elements a batch of `count` needs: one group's worth (0 for one-step plans)
inline size_t ntt_batch_scratch_elems(uint32_t log_n, size_t count) {
  if (!ntt_batch_log_ok(log_n) || log_n <= NTT_BATCH_ONE_STEP_MAX_LOG) return 0;
  const size_t per = ntt_batch_per_launch(log_n);
  return (count < per ? count : per) << log_n;
}

// Element strides between two transforms of a group at step i of an nsteps-step plan (ntt_step_args: which of data / scratch the
// step reads and writes): a single step works on the caller's array in place, step A reads it and writes scratch, step B (three-step
// plans) works on scratch in place, the last step reads scratch and writes the caller's array.
struct NttBatchStrides { size_t in, out; };
inline NttBatchStrides ntt_batch_step_strides(int nsteps, int i, size_t n, size_t stride) {
  if (nsteps == 1) return {stride, stride};
  if (i == 0) return {stride, n};
  if (i < nsteps - 1) return {n, n};
  return {n, stride};
}

// the argument checks of both batched entries (true = acceptable); count == 0 is acceptable (nothing is enqueued)
inline bool ntt_batch_args_ok(const void* ctx, const void* d_data, uint32_t log_n, size_t count, size_t stride) {
  if (!ctx || !d_data || !ntt_batch_log_ok(log_n)) return false;
  if (stride < ((size_t)1 << log_n)) return false;
  if (count != 0 && stride > SIZE_MAX / 32 / count) return false;       // count * stride elements of 32 bytes must fit a size_t
  return true;
}

}  // namespace kg
