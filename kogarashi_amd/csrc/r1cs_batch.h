// r1cs_batch.h -- the host-only, pure parts of the batched CSR product (kg_r1cs_prod_batch, vec.hip) and of the batched prover's R1CS form
// (kg_groth16_prove_r1cs_batch, groth16_batch.hip): how a batch of vectors is cut into launches and the argument checks; at the end of the
// file the same for the batched check (kg_r1cs_check_batch, kg_groth16_witness_check_batch, vec.hip) and for the batched cross term
// (kg_nova_cross_term_batch, vec.hip).  No HIP, no context: tests/host/r1cs_batch_host.cpp, tests/host/r1cs_check_batch_host.cpp and
// tests/host/nova_fold_batch_host.cpp include this file alone.
//
// Layout: vector b of a batch is read at elements [b * z_stride, ...) of d_z (its length is whatever the matrix's columns index: the call
// cannot know it) and its m row sums go to elements [b * out_stride, b * out_stride + m) of d_out (out_stride >= m, elements of 4 words);
// the elements between two outputs are neither read nor written.  The vector index is a launch's grid y dimension, so a batch is cut into
// chunks of at most R1CS_BATCH_GRID_Y_MAX vectors; the work list of long rows depends on the matrix alone and is built by the first chunk.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include "groth16_batch.h"

namespace kg {

// The row classes of the sparse-row walker (vec.hip): a row of up to SHORT_ROW entries is summed by one lane, a longer one by a wave, one of
// more than HUGE_ROW by a 1024-lane workgroup (the constant-one wire's row of a transposed system: an entry per constraint)
constexpr uint32_t SHORT_ROW = 48;
constexpr uint32_t HUGE_ROW = 4096;

constexpr size_t R1CS_BATCH_GRID_Y_MAX = 65535;       // a HIP grid's y dimension carries at most 65535 blocks

// number of launches' worth a batch of `count` vectors is cut into (0 for an empty batch); chunks run one after another on the stream
inline size_t r1cs_batch_chunks(size_t count) { return count == 0 ? 0 : (count - 1) / R1CS_BATCH_GRID_Y_MAX + 1; }
// chunk i of the batch: vectors [first, first + count)
struct R1csBatchChunk { size_t first, count; };
inline R1csBatchChunk r1cs_batch_chunk(size_t count, size_t i) {
  const size_t first = i * R1CS_BATCH_GRID_Y_MAX;
  return {first, count - first < R1CS_BATCH_GRID_Y_MAX ? count - first : R1CS_BATCH_GRID_Y_MAX};
}
// Blocks in x of the second and third launch (a wave / a workgroup per (list entry, vector)): the single product's `single` blocks spread
// over the chunk's vectors, at least one -- the list's length is on the device only, so the grid is sized by what is known on the host
inline unsigned r1cs_batch_grid_x(unsigned single, size_t chunk_count) {
  const size_t x = chunk_count == 0 ? single : single / chunk_count;
  return x < 1 ? 1u : (unsigned)x;
}

inline bool r1cs_batch_field_ok(int field) { return field == 0 || field == 1; }       // KG_FR, KG_FQ

// The argument checks of kg_r1cs_prod_batch (true = acceptable), made before anything is dereferenced.  An empty call (count == 0 or
// m == 0, r1cs_batch_empty) is acceptable with any array pointers; a null ctx, an unknown field, out_stride < m and m >= 2^32 are not
// acceptable even then.
inline bool r1cs_batch_empty(size_t m, size_t count) { return m == 0 || count == 0; }
inline bool r1cs_batch_args_ok(const void* ctx, int field, const void* d_row_ptr, const void* d_col, const void* d_val, size_t m, const void* d_z,
                               size_t z_stride, size_t count, const void* d_out, size_t out_stride) {
  if (!ctx || !r1cs_batch_field_ok(field)) return false;
  if (out_stride < m || m >= ((uint64_t)1 << 32)) return false;
  if (r1cs_batch_empty(m, count)) return true;
  if (!d_row_ptr || !d_col || !d_val || !d_z || !d_out) return false;
  if (z_stride > SIZE_MAX / 32 / count || out_stride > SIZE_MAX / 32 / count) return false;      // count * stride elements of 32 bytes
  return true;
}

// The argument checks of kg_groth16_prove_r1cs_batch: those of kg_groth16_prove_batch with the three matrices in the place of the three
// evaluation arrays (Csr: anything with d_row_ptr, d_col, d_val).  A null matrix or member array is refused when count > 0.
template <class Csr>
inline bool g16_r1cs_batch_args_ok(const void* ctx, const void* crs, size_t m, size_t l, size_t m_l_1, const Csr* a, const Csr* b, const Csr* c, const void* d_x,
                                   size_t x_stride, const void* d_w, size_t w_stride, const void* d_r, const void* d_s, size_t count, const void* d_proofs,
                                   const void* d_inf) {
  const void* some = ctx;                                  // stands for the evaluation arrays, with a stride of exactly m
  if (!g16_batch_args_ok(ctx, crs, m, l, m_l_1, some, some, some, m, d_x, x_stride, d_w, w_stride, d_r, d_s, count, d_proofs, d_inf)) return false;
  if (count == 0) return true;
  for (const Csr* x : {a, b, c})
    if (!x || !x->d_row_ptr || !x->d_col || !x->d_val) return false;
  return true;
}

// ---- the batched satisfiability check (kg_r1cs_check_batch, kg_groth16_witness_check_batch; vec.hip CheckOp) -------------------------
// Layout: vector b is read at element b * z_stride of d_z (or x_b at b * x_stride of d_x and w_b at b * w_stride of d_w), E_b at element
// b * e_stride of d_e, u_b is element b of d_u; row i's status byte goes to d_status[b * status_stride + i] (a stride in BYTES) and the
// vector's summary pair (bad rows, smallest bad row or m) to words 2 b and 2 b + 1 of d_summary.  The chunk rule is the product's.
constexpr size_t r1cs_check_batch_summary_word(size_t vec) { return 2 * vec; }
constexpr size_t r1cs_check_batch_status_byte(size_t vec, size_t status_stride, size_t row) { return vec * status_stride + row; }

// The split source's index rule: column j of z = x || w is x[j] for j < l and w[j - l] otherwise (SparseMatrix::prod's wire arithmetic,
// zkstd/src/matrix.rs:36-48).  constexpr: the kernels call the very function the host test checks.
struct R1csSplitAt { bool in_x; size_t index; };
constexpr R1csSplitAt r1cs_split_at(size_t j, size_t l) { return {j < l, j < l ? j : j - l}; }

template <class Csr>
inline bool r1cs_csr3_ok(const Csr* a, const Csr* b, const Csr* c) {
  for (const Csr* x : {a, b, c})
    if (!x || !x->d_row_ptr || !x->d_col || !x->d_val) return false;
  return true;
}

// The argument checks of kg_r1cs_check_batch (true = acceptable), made before anything is dereferenced or enqueued.  count == 0 is
// acceptable with any pointers, m == 0 with any but d_summary (every pair becomes (0, 0)); a null ctx, an unknown field and m >= 2^32 are not
// acceptable even then.  status_stride counts bytes, the other strides elements of 32 bytes.
template <class Csr>
inline bool r1cs_check_batch_args_ok(const void* ctx, int field, const Csr* a, const Csr* b, const Csr* c, size_t m, const void* d_z, size_t z_stride,
                                     size_t count, const void* d_e, size_t e_stride, const void* d_status, size_t status_stride, const void* d_summary) {
  if (!ctx || !r1cs_batch_field_ok(field) || m >= ((uint64_t)1 << 32)) return false;
  if (count == 0) return true;
  if (!d_summary || count > SIZE_MAX / 8) return false;                                  // count pairs of 32-bit words
  if (m == 0) return true;
  if (!r1cs_csr3_ok(a, b, c) || !d_z) return false;
  if ((d_e && e_stride < m) || (d_status && status_stride < m)) return false;
  if (z_stride > SIZE_MAX / 32 / count || (d_e && e_stride > SIZE_MAX / 32 / count) || (d_status && status_stride > SIZE_MAX / count)) return false;
  return true;
}

// The argument checks of kg_groth16_witness_check_batch: l >= 1, x_stride >= l and w_stride >= m_l_1 are refused even for an empty call (as
// g16_batch_args_ok refuses them); d_w may be null when the circuit has no witness wire.
template <class Csr>
inline bool g16_witness_check_batch_args_ok(const void* ctx, const Csr* a, const Csr* b, const Csr* c, size_t m, size_t l, size_t m_l_1, const void* d_x,
                                            size_t x_stride, const void* d_w, size_t w_stride, size_t count, const void* d_status, size_t status_stride,
                                            const void* d_summary) {
  if (!ctx || m >= ((uint64_t)1 << 32) || l < 1 || x_stride < l || w_stride < m_l_1) return false;
  if (count == 0) return true;
  if (!d_summary || count > SIZE_MAX / 8) return false;
  if (m == 0) return true;
  if (!r1cs_csr3_ok(a, b, c) || !d_x || (m_l_1 && !d_w)) return false;
  if (d_status && status_stride < m) return false;
  if (x_stride > SIZE_MAX / 32 / count || w_stride > SIZE_MAX / 32 / count || (d_status && status_stride > SIZE_MAX / count)) return false;
  return true;
}

// ---- the batched Nova cross term (kg_nova_cross_term_batch; vec.hip CrossOp) -------------------------------------------------------
// Layout: pair b reads z1_b at element b * z1_stride of d_z1 and z2_b at element b * z2_stride of d_z2 and writes the m elements of T_b at
// element b * out_stride of d_out (out_stride >= m); u1_b and u2_b are element b of d_u1 / d_u2 (null: one for every pair -- not looked at
// here).  The chunk rule is the product's.
// The argument checks (true = acceptable), made before anything is dereferenced or enqueued.  An empty call (count == 0 or m == 0) is
// acceptable with any pointers; a null ctx, an unknown field, m >= 2^32 and out_stride < m are not acceptable even then.
template <class Csr>
inline bool nova_cross_batch_args_ok(const void* ctx, int field, const Csr* a, const Csr* b, const Csr* c, size_t m, const void* d_z1, size_t z1_stride,
                                     const void* d_z2, size_t z2_stride, size_t count, const void* d_out, size_t out_stride) {
  if (!ctx || !r1cs_batch_field_ok(field) || m >= ((uint64_t)1 << 32) || out_stride < m) return false;
  if (r1cs_batch_empty(m, count)) return true;
  if (!r1cs_csr3_ok(a, b, c) || !d_z1 || !d_z2 || !d_out) return false;
  if (z1_stride > SIZE_MAX / 32 / count || z2_stride > SIZE_MAX / 32 / count || out_stride > SIZE_MAX / 32 / count) return false;
  return true;
}

}  // namespace kg
