// nova_batch.h -- the host-only, pure parts of the two smaller primitives of a batched Nova fold: the axpy with a scalar per vector
// (kg_field_vec_axpy_batch, vec.hip) and P + k Q for many points (kg_points_muladd_batch, points_fold.hip).  The cross term's are in
// r1cs_batch.h.  No HIP, no context: tests/host/nova_fold_batch_host.cpp includes this file alone.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

namespace kg {

// ---- kg_field_vec_axpy_batch ---------------------------------------------------------------------------------------------------------------
// Layout: vector b reads a_b at element b * a_stride of d_a and b_b at element b * b_stride of d_b, its scalar is element b of d_s, and its
// n results go to element b * out_stride of d_out; the elements between two vectors are neither read nor written.  One lane per
// (vector, element): lane t of the call takes element t % n of vector t / n.
struct AxpyBatchAt { size_t vec, elem; };
constexpr AxpyBatchAt axpy_batch_at(size_t t, size_t n) { return {t / n, t % n}; }
// a launch carries at most this many lanes (2^30 blocks of 256); a longer call is cut into launches one after another
constexpr size_t AXPY_BATCH_LAUNCH_MAX = (size_t)1 << 38;

inline bool axpy_batch_empty(size_t n, size_t count) { return n == 0 || count == 0; }
// The argument checks (true = acceptable), made before anything is dereferenced or enqueued.  An empty call (n == 0 or count == 0) is
// acceptable with any pointers; a null ctx, an unknown field and a stride below n are not acceptable even then.
inline bool axpy_batch_args_ok(const void* ctx, int field, const void* d_a, size_t a_stride, const void* d_s, const void* d_b, size_t b_stride,
                               const void* d_out, size_t out_stride, size_t n, size_t count) {
  if (!ctx || (field != 0 && field != 1)) return false;                              // KG_FR, KG_FQ
  if (a_stride < n || b_stride < n || out_stride < n) return false;
  if (axpy_batch_empty(n, count)) return true;
  if (!d_a || !d_s || !d_b || !d_out) return false;
  if (a_stride > SIZE_MAX / 32 / count || b_stride > SIZE_MAX / 32 / count || out_stride > SIZE_MAX / 32 / count) return false;      // count * stride * 32 bytes
  return true;
}

// ---- kg_points_muladd_batch ----------------------------------------------------------------------------------------------------------------
// out_j = P_j + k_{j / per_scalar} Q_j: consecutive groups of per_scalar points share a scalar (a Nova fold: commit_w and commit_e, one r)
constexpr size_t points_muladd_scalar_at(size_t j, size_t per_scalar) { return j / per_scalar; }
constexpr size_t POINTS_MULADD_MAX = (size_t)1 << 37;           // one lane per point, 64 per block: the grid's x dimension

// The argument checks (true = acceptable), made before anything is dereferenced or enqueued.  count == 0 is acceptable with any pointers;
// a null ctx, a curve other than KG_G1 (0) and KG_GRUMPKIN (1) and per_scalar == 0 are not acceptable even then.  The flag arrays of the
// operands may be null (no identities); the result's may not.
inline bool points_muladd_args_ok(const void* ctx, int curve, const void* d_p_xy, const void* d_q_xy, const void* d_k, size_t per_scalar, size_t count,
                                  const void* d_out_xy, const void* d_out_inf) {
  if (!ctx || (curve != 0 && curve != 1) || per_scalar < 1) return false;
  if (count == 0) return true;
  if (!d_p_xy || !d_q_xy || !d_k || !d_out_xy || !d_out_inf) return false;
  if (count >= POINTS_MULADD_MAX) return false;
  return true;
}

}  // namespace kg
