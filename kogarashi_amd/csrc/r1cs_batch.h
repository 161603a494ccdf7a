// r1cs_batch.h -- the host-only, pure parts of the batched CSR product (kg_r1cs_prod_batch, vec.hip) and of the batched prover's R1CS form
// (kg_groth16_prove_r1cs_batch, groth16_batch.hip): how a batch of vectors is cut into launches and the argument checks.  No HIP, no
// context: tests/host/r1cs_batch_host.cpp includes this file alone.
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

}  // namespace kg
