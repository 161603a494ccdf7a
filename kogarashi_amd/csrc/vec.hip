// vec.hip -- element-wise field kernels and the deterministic synthetic-input generators.
//
// kg_field_vec_op replaces, one GPU thread per element, the reference's limb functions
// zkstd/src/arithmetic/limbs/bits_256/normal.rs:4-31,34-53,56-80,83-121,124-166,170-184,256-270 and the
// point-wise polynomial ops groth16/src/poly.rs:168-195.  HBM-bound for add/sub/mul (96 B/element).
#include <type_traits>
#include "common.h"
#include "vecops.h"
#include "host_fp.h"
#include "r1cs_batch.h"
#include "nova_batch.h"

using namespace kg;

namespace {

template <class P>
__global__ void __launch_bounds__(256) k_vec_op(int op, const uint64_t* a, const uint64_t* b,
                                                uint64_t* out, size_t n) {
  KG_SERVICE_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wa[8], wb[8], wo[8];
  load_words(a, i, wa);
  const bool binary = (op == KG_OP_ADD || op == KG_OP_SUB || op == KG_OP_MUL);
  if (binary) load_words(b, i, wb);
  using F = Fp<P>;
  // The linear ops never leave the caller's Montgomery domain (a*R + b*R = (a+b)*R): re-pack, lazy add / fat subtract,
  // one value reduction, canonicalise.  A product needs one extra constant product: mont'(aR, bR) = ab*R^2/2^261, and
  // mont'(., 2^522/R) brings it back to ab*R.
  const F A = limbs_from_words<P>(wa);
  switch (op) {
    case KG_OP_ADD: words_from_limbs(reduce_2p(vred(norm(add(A, limbs_from_words<P>(wb))))), wo); break;
    case KG_OP_SUB: words_from_limbs(reduce_2p(vred(norm(sub<8, 1>(A, limbs_from_words<P>(wb))))), wo); break;
    case KG_OP_MUL: words_from_limbs(reduce_2p(mul(mul(A, limbs_from_words<P>(wb)), F::from_const(P::C_FROM_REF))), wo); break;
    case KG_OP_SQUARE: words_from_limbs(reduce_2p(mul(sqr(A), F::from_const(P::C_FROM_REF))), wo); break;
    case KG_OP_NEG: words_from_limbs(reduce_2p(vred(norm(sub<8, 1>(F::zero(), A)))), wo); break;
    case KG_OP_DOUBLE: words_from_limbs(reduce_2p(vred(norm(dbl(A)))), wo); break;
    case KG_OP_INVERT: to_ref(inv_fast(from_ref<P>(wa)), wo); break;
    case KG_OP_FROM_MONT: ref_to_int<P>(wa, wo); break;
    case KG_OP_TO_MONT: int_to_ref<P>(wa, wo); break;
    default: return;
  }
  store_words(out, i, wo);
}

template <class P>
__global__ void __launch_bounds__(256) k_vec_scale(const uint64_t* a, Words8 s, uint64_t* out, size_t n) {
  KG_SERVICE_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wa[8], wo[8];
  load_words(a, i, wa);
  // data stays in the caller's Montgomery domain: multiply by the constant in internal form
  Fp<P> sc = from_ref<P>(s.w);
  words_from_limbs(reduce_2p(mul(limbs_from_words<P>(wa), sc)), wo);
  store_words(out, i, wo);
}

// out[i] = start * base^i: each lane raises base to its own index (<= 64 squarings), no serial scan
template <class P>
__global__ void __launch_bounds__(256) k_powers(Words8 start, Words8 base, uint64_t* __restrict__ out, size_t n) {
  KG_SERVICE_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fp<P> b = from_ref<P>(base.w), r = from_ref<P>(start.w);
  for (size_t e = i; e; e >>= 1) {
    if (e & 1) r = mul(r, b);
    b = sqr(b);
  }
  uint32_t wo[8];
  to_ref(r, wo);
  store_words(out, i, wo);
}

// out = a + s * b  (Nova fold, witness.rs:56-70): one product, lazy sum, one canonicalisation per element
template <class P>
__global__ void __launch_bounds__(256) k_vec_axpy(const uint64_t* a, Words8 s, const uint64_t* b,
                                                  uint64_t* out, size_t n) {
  KG_SERVICE_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wa[8], wb[8], wo[8];
  load_words(a, i, wa);
  load_words(b, i, wb);
  // raw(b) * internal(s) stays in the ABI's Montgomery domain, like raw(a)  (vecops.h axpy_step)
  words_from_limbs(reduce_2p(axpy_step(limbs_from_words<P>(wa), limbs_from_words<P>(wb), from_ref<P>(s.w))), wo);
  store_words(out, i, wo);
}
// out_b = a_b + s_b * b_b for the vectors of a batch (kg_field_vec_axpy_batch): a lane per (vector, element) over the flattened index, so
// that short vectors fill their waves and no grid dimension bounds the count; s_b is read from the device, one element per vector.
// out may be a: every lane reads its own element before it writes it.
template <class P>
__global__ void __launch_bounds__(256) k_vec_axpy_batch(const uint64_t* a, size_t a_stride, const uint64_t* __restrict__ s, const uint64_t* __restrict__ b,
                                                        size_t b_stride, uint64_t* out, size_t out_stride, size_t n, size_t first, size_t total) {
  KG_SERVICE_PRIO();
  const size_t t = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const AxpyBatchAt at = axpy_batch_at(t, n);
  uint32_t wa[8], wb[8], ws[8], wo[8];
  load_words(a, at.vec * a_stride + at.elem, wa);
  load_words(b, at.vec * b_stride + at.elem, wb);
  load_words(s, at.vec, ws);
  words_from_limbs(reduce_2p(axpy_step(limbs_from_words<P>(wa), limbs_from_words<P>(wb), from_ref<P>(ws))), wo);
  store_words(out, at.vec * out_stride + at.elem, wo);
}

// CSR sparse matrix-vector product (zkstd/src/matrix/row.rs:43-51, matrix.rs:36-48), G lanes per row: lanes stride over the
// row's entries, partial sums meet through log2(G) shuffle steps.  G = 1 (a lane per row) for constraint rows, G = 64 (a
// wave per row) for the long rows of kg_r1cs_prod's work list.
template <class P>
__device__ __forceinline__ Fp<P> shfl_xor_f(const Fp<P>& a, int mask) {
  Fp<P> r;
#pragma unroll
  for (int k = 0; k < 9; ++k) r.l[k] = __shfl_xor(a.l[k], mask);
  return r;
}
// sum_e val[e] * z[col[e]] over the row, for one or two z vectors (every lane of the group holds the result).  Both factors are
// used as they lie in memory (x * 2^256), so a term is ONE Montgomery product -- z * val * 2^251 -- and the sums live in that
// "raw product" domain; the caller's next multiplication carries the constant that leaves it (C_FROM_REF for a plain
// matrix-vector product, the folded constants of cross_term_row).  Converting each coefficient first cost a second product per entry.
// Z: where the vector's entries come from -- a pointer to its elements, or the batched witness check's split x | w (ZSplit).
__device__ __forceinline__ void load_z(const uint64_t* __restrict__ z, uint64_t c, uint32_t w[8]) { load_words(z, c, w); }
struct ZSplit { const uint64_t* x; const uint64_t* w; size_t l; };          // z = x || w read in place: column j is x[j] for j < l, w[j - l] otherwise
__device__ __forceinline__ void load_z(const ZSplit& z, uint64_t c, uint32_t w[8]) {
  const R1csSplitAt at = r1cs_split_at(c, z.l);              // one compare and two selects per entry; one load either way
  load_words(at.in_x ? z.x : z.w, at.index, w);
}
template <class P, int G, int NZ, class Z>
__device__ __forceinline__ void row_dot(const uint64_t* __restrict__ row_ptr, const uint64_t* __restrict__ col, const uint64_t* __restrict__ val,
                                        size_t row, int lane, const Z& z1, const Z& z2, Fp<P> (&sum)[NZ]) {
#pragma unroll
  for (int q = 0; q < NZ; ++q) sum[q] = Fp<P>::zero();
  for (uint64_t e = row_ptr[row] + lane; e < row_ptr[row + 1]; e += G) {
    uint32_t wv[8], wz[8];
    load_words(val, e, wv);
    const Fp<P> v = limbs_from_words<P>(wv);
    const uint64_t c = col[e];
    load_z(z1, c, wz);
    sum[0] = dot_step(sum[0], limbs_from_words<P>(wz), v);
    if (NZ > 1) {
      load_z(z2, c, wz);
      sum[NZ - 1] = dot_step(sum[NZ - 1], limbs_from_words<P>(wz), v);
    }
  }
  if (G > 1) {
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1)
#pragma unroll
      for (int q = 0; q < NZ; ++q) sum[q] = dot_merge(sum[q], shfl_xor_f(sum[q], d));
  }
}

// The sparse-row scheme, once for the matrix-vector product, Nova's cross term and the satisfiability check: two launches.  Constraint rows
// hold a handful of terms (1.3 per matrix in the chain circuit), so a lane takes a whole row (k_rows_lane): a wave per row kept 63 of 64
// lanes idle (0.45 ms per 2^18-row product), 8 lanes per row ran the cross term at 230 GB/s of algorithmic traffic (1.17 ms at 2^20 rows,
// instruction-bound) and paid shuffle-tree merges for nothing.  A row of more than SHORT_ROW terms -- a range check's bit sum: 254; the
// transposed systems of the setup have one per heavily used wire, the constant-one wire touching every constraint -- would hold its whole
// wave for ~0.5 us per term and z vector: it is put on a work list instead and gets a whole wave in the second launch (k_rows_wave).
// What a row is and does comes from the operation Op:
//   int klass(row)                       0: a lane takes the row; 1: the list's front (a wave); 2: the list's back (a workgroup: the product's
//                                        k_r1cs_rows_huge).  It depends on the matrix alone.
//   template <int G> bool row(row, lane, b)   the row of vector b by G lanes -- G = 1: lane = 0; G = 64: every lane of the wave, lane 0 finishes;
//                                        true (lane 0 only): the row is bad
//   REPORTS, uint32_t* summary(b)        bad rows are folded into vector b's pair: the lowest bad lane speaks for its 64 rows, a wave of
//                                        k_rows_wave for the rows it took (the list is in no particular order)
// One call runs the operation against `count` vectors (launch_rows): the vector is the block's y index b, and the single calls are the batch
// of one.  A lane per (short row, vector), a wave per (list entry, vector).  The work list is the matrix's, so it is built once per call: by
// the y = 0 blocks of the launch that `lists` (the first chunk's).  Every other lane that meets a long row leaves it to the list's launches;
// trip counts stay wave-uniform, the list and its counters being the same for every y.
struct CsrView {
  const uint64_t* row_ptr; const uint64_t* col; const uint64_t* val;
  __device__ __forceinline__ uint64_t len(size_t row) const { return row_ptr[row + 1] - row_ptr[row]; }
};
template <class Op>
__global__ void __launch_bounds__(256) k_rows_lane(Op op, size_t m, RowWs ws, bool lists) {
  KG_SERVICE_PRIO();
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  bool bad = false;                                       // lanes past the end and lanes whose row is a work list's report nothing
  if (row < m) {
    const int k = op.klass(row);
    if (k == 0) bad = op.template row<1>(row, 0, b);
    else if (lists && b == 0) {
      if (k == 2) ws.list[m - 1 - atomicAdd(ws.count + 1, 1u)] = (uint32_t)row;
      else ws.list[atomicAdd(ws.count, 1u)] = (uint32_t)row;
    }
  }
  if constexpr (Op::REPORTS) summary_fold(op.summary(b), bad, (uint32_t)row);
}
// (the list as const __restrict__ parameters: handed over as a RowWs, the cross term's and the check's instances take one VGPR more)
template <class Op>
__global__ void __launch_bounds__(256) k_rows_wave(Op op, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count) {
  KG_SERVICE_PRIO();
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6), wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const size_t b = blockIdx.y;
  const uint32_t total = *count;
  uint32_t n_bad = 0, first = 0xffffffffu;                // lane 0 keeps them
  for (uint32_t i = wave; i < total; i += nwaves) {      // wave-uniform trip count: the shuffles inside row_dot see full waves
    const size_t row = list[i];
    if (op.template row<64>(row, lane, b)) { ++n_bad; first = min(first, (uint32_t)row); }
  }
  if constexpr (Op::REPORTS)
    if (lane == 0 && n_bad != 0) summary_add(op.summary(b), n_bad, first);
}

// A HUGE row (more than HUGE_ROW entries) per WORKGROUP: 1024 lanes stride over its entries; wave sums by shuffles, the sixteen wave sums
// through LDS.  Up to round 4 a wave took every long row: the transposed systems of the setup have a row per wire, and the constant-one wire's
// row holds an entry per constraint -- 2^18 entries on 64 lanes took 4.8 ms of a 29 ms setup.  Rows of 49 .. 4096 entries (a range check's bit
// sum: 254) keep a wave each: a circuit may hold tens of thousands of them, and 1024 waves take them in parallel.
// A workgroup per (list entry, vector), the vector is the block's y index (strides in elements).
constexpr int LONG_NT = 1024;
template <class P>
__global__ void __launch_bounds__(LONG_NT) k_r1cs_rows_huge(const uint64_t* __restrict__ row_ptr, const uint64_t* __restrict__ col,
                                                            const uint64_t* __restrict__ val, const uint64_t* __restrict__ z, size_t z_stride,
                                                            uint64_t* __restrict__ out, size_t out_stride, const uint32_t* __restrict__ long_rows,
                                                            const uint32_t* __restrict__ long_count, size_t m) {
  KG_SERVICE_PRIO();
  __shared__ uint32_t part[LONG_NT / 64][9];
  z += (size_t)blockIdx.y * z_stride * 4;
  out += (size_t)blockIdx.y * out_stride * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t total = long_count[1];
  for (uint32_t i = blockIdx.x; i < total; i += gridDim.x) {      // workgroup-uniform trip count
    const size_t row = long_rows[m - 1 - i];
    Fp<P> sum = Fp<P>::zero();
    for (uint64_t e = row_ptr[row] + threadIdx.x; e < row_ptr[row + 1]; e += LONG_NT) {
      uint32_t wv[8], wz[8];
      load_words(val, e, wv);
      load_words(z, col[e], wz);
      sum = dot_step(sum, limbs_from_words<P>(wz), limbs_from_words<P>(wv));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum = dot_merge(sum, shfl_xor_f(sum, d));
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) part[wave][k] = sum.l[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      Fp<P> tot = sum;                                          // wave 0's own sum
      for (int w = 1; w < LONG_NT / 64; ++w) {
        Fp<P> o;
#pragma unroll
        for (int k = 0; k < 9; ++k) o.l[k] = part[w][k];
        tot = dot_merge(tot, o);
      }
      uint32_t wo[8];
      words_from_limbs(reduce_2p(mul(tot, Fp<P>::from_const(P::C_FROM_REF))), wo);
      store_words(out, row, wo);
    }
    __syncthreads();
  }
}

// out_b = M z_b  (zkstd/src/matrix/row.rs:43-51, matrix.rs:36-48): long rows to the list's front, huge rows to its back.  Vector b is read at
// element b * z_stride of z, its row sums go to element b * out_stride of out.
template <class P>
struct ProdOp {
  static constexpr bool REPORTS = false;
  CsrView M; const uint64_t* z; size_t z_stride; uint64_t* out; size_t out_stride;
  __device__ __forceinline__ int klass(size_t row) const { const uint64_t len = M.len(row); return len > HUGE_ROW ? 2 : (len > SHORT_ROW ? 1 : 0); }
  template <int G>
  __device__ __forceinline__ bool row(size_t row, int lane, size_t b) const {
    const uint64_t* zb = z + b * z_stride * 4;
    Fp<P> sum[1];
    row_dot<P, G, 1>(M.row_ptr, M.col, M.val, row, lane, zb, zb, sum);
    if (lane == 0) {
      uint32_t wo[8];
      words_from_limbs(reduce_2p(mul(sum[0], Fp<P>::from_const(P::C_FROM_REF))), wo);        // raw product domain -> the ABI's
      store_words(out, b * out_stride + row, wo);
    }
    return false;
  }
};

// The two operations over a whole R1CS: a row is long when it has more than SHORT_ROW entries in ANY of the three matrices; every matrix row
// is read once, for one or two z vectors, and the row sums never touch memory
struct Csr3 {
  CsrView A, B, C;
  __device__ __forceinline__ int klass(size_t row) const { return A.len(row) > SHORT_ROW || B.len(row) > SHORT_ROW || C.len(row) > SHORT_ROW; }
  template <class P, int G, int NZ, class Z>
  __device__ __forceinline__ void dots(size_t row, int lane, const Z& z1, const Z& z2, Fp<P> (&az)[NZ], Fp<P> (&bz)[NZ], Fp<P> (&cz)[NZ]) const {
    row_dot<P, G, NZ>(A.row_ptr, A.col, A.val, row, lane, z1, z2, az);
    row_dot<P, G, NZ>(B.row_ptr, B.col, B.val, row, lane, z1, z2, bz);
    row_dot<P, G, NZ>(C.row_ptr, C.col, C.val, row, lane, z1, z2, cz);
  }
};
// A u per vector in the factor form the row functions want next to raw row sums, u * 2^266: element b of `u` (the ABI form) scaled on the
// device (u_factor), or, when the call has no such array, `us`: one value for every vector, scaled on the host (scaled()).  Both are
// representatives of one residue and the row is canonicalised at the end, so the two ways give the same words.
// DEV_U = false: the call has no arrays at all, and the kernel no load and no select (the single cross term's wave kernel keeps its time so).
struct Limbs9 { uint32_t l[9]; };
template <class P, bool DEV_U = true>
__device__ __forceinline__ Fp<P> u_of(const uint64_t* u, const Limbs9& us, size_t b) {
  if (!DEV_U || u == nullptr) return Fp<P>::from_const(us.l);
  uint32_t wu[8];
  load_words(u, b, wu);
  return u_factor(limbs_from_words<P>(wu), Fp<P>::from_const(P::C_XT_U));
}

// Nova's cross term (nova/src/prover.rs:53-90): T = AZ1 o BZ2 + AZ2 o BZ1 - u1 * CZ2 - u2 * CZ1; bound by its ~12 products per row.
// Pair b reads z1_b, z2_b at elements b * z1_stride, b * z2_stride and writes T_b at element b * out_stride.  kg_nova_cross_term hands in
// its two host-scaled u and no arrays (DEV_U = false), kg_nova_cross_term_batch its arrays (each may be null: u = 1, the host-scaled one).
template <class P, bool DEV_U>
struct CrossOp : Csr3 {
  static constexpr bool REPORTS = false;
  const uint64_t* z1; size_t z1_stride; const uint64_t* z2; size_t z2_stride; const uint64_t *u1, *u2; Limbs9 us1, us2; uint64_t* out; size_t out_stride;
  template <int G>
  __device__ __forceinline__ bool row(size_t row, int lane, size_t b) const {
    Fp<P> az[2], bz[2], cz[2];
    dots<P, G, 2>(row, lane, z1 + b * z1_stride * 4, z2 + b * z2_stride * 4, az, bz, cz);
    if (lane == 0) {
      const Fp<P> r = cross_term_row(az[0], az[1], bz[0], bz[1], cz[0], cz[1], u_of<P, DEV_U>(u1, us1, b), u_of<P, DEV_U>(u2, us2, b),
                                     Fp<P>::from_const(P::C_XT_HAD));
      uint32_t wo[8];
      words_from_limbs(reduce_2p(r), wo);
      store_words(out, b * out_stride + row, wo);
    }
    return false;
  }
};

// kg_r1cs_check, kg_r1cs_check_batch, kg_groth16_witness_check_batch: is (A z)_i (B z)_i = u (C z)_i + E_i for every row?
// (nova/src/relaxed_r1cs.rs:81-114 is_sat_relaxed; u = 1 and E = 0: zkstd/src/r1cs.rs:62-77 is_sat.)  The shape of the cross term with one z
// vector; instead of an element per row it leaves a status byte (when asked) and the vector's summary pair (common.h; row indices are
// below 2^32).  Every vector folds into its own pair of `sums`, so a lane of k_rows_lane speaks for its 64 rows of vector b and a wave of
// k_rows_wave for the rows it took of that vector: at most one atomicAdd / atomicMin pair per wave and launch, spread over count addresses.
// Z: the vectors' source, vec(b) is what row_dot reads vector b through (the single call: ZStrided{d_z, 0}, and sums is the work space's
// pair).  e == nullptr: E = 0, nothing is read.  Strides in elements, status_stride in bytes.
struct ZStrided {
  const uint64_t* z; size_t stride;
  __device__ __forceinline__ const uint64_t* vec(size_t b) const { return z + b * stride * 4; }
  ZStrided from(size_t first) const { return {z + first * stride * 4, stride}; }
};
struct ZSplitStrided {
  const uint64_t* x; size_t x_stride; const uint64_t* w; size_t w_stride, l;
  __device__ __forceinline__ ZSplit vec(size_t b) const { return {x + b * x_stride * 4, w + b * w_stride * 4, l}; }
  ZSplitStrided from(size_t first) const { return {x + first * x_stride * 4, x_stride, w + first * w_stride * 4, w_stride, l}; }
};
template <class P, class Z>
struct CheckOp : Csr3 {
  static constexpr bool REPORTS = true;
  Z z; const uint64_t* u; Limbs9 us; const uint64_t* e; size_t e_stride; uint8_t* status; size_t status_stride; uint32_t* sums;
  __device__ __forceinline__ uint32_t* summary(size_t b) const { return sums + r1cs_check_batch_summary_word(b); }
  template <int G>
  __device__ __forceinline__ bool row(size_t row, int lane, size_t b) const {
    const auto zb = z.vec(b);
    Fp<P> az[1], bz[1], cz[1];
    dots<P, G, 1>(row, lane, zb, zb, az, bz, cz);
    if (lane != 0) return false;
    Fp<P> er = Fp<P>::zero();
    if (e != nullptr) {
      uint32_t we[8];
      load_words(e, b * e_stride + row, we);
      er = limbs_from_words<P>(we);
    }
    const bool bad = !is_zero_mod_p(sat_residual_row(az[0], bz[0], cz[0], u_of<P>(u, us, b), er, Fp<P>::from_const(P::C_XT_HAD)));
    if (status != nullptr) status[r1cs_check_batch_status_byte(b, status_stride, row)] = bad ? (uint8_t)KG_ROW_UNSAT : (uint8_t)0;
    return bad;
  }
};
// the check's one initialising launch: every vector's pair to (0, m), and the two list counters
__global__ void __launch_bounds__(256) k_check_batch_init(uint32_t* __restrict__ sums, size_t count, uint32_t m, uint32_t* __restrict__ counters) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0 && counters != nullptr) { counters[0] = 0; counters[1] = 0; }      // (no rows: no list, no counters)
  if (b < count) { sums[2 * b] = 0; sums[2 * b + 1] = m; }
}

// ---- splitmix64 streams (oracle/pyoracle.py stream_at, oracle/kg_oracle.c stream_words) ---------------
__device__ __forceinline__ uint64_t splitmix_next(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ULL;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__device__ __forceinline__ void stream_words(uint64_t seed, uint64_t index, uint32_t lo[8], uint32_t hi[8]) {
  uint64_t s = seed + 8 * index * 0x9E3779B97F4A7C15ULL;
#pragma unroll
  for (int i = 0; i < 4; ++i) { uint64_t v = splitmix_next(s); lo[2 * i] = (uint32_t)v; lo[2 * i + 1] = (uint32_t)(v >> 32); }
#pragma unroll
  for (int i = 0; i < 4; ++i) { uint64_t v = splitmix_next(s); hi[2 * i] = (uint32_t)v; hi[2 * i + 1] = (uint32_t)(v >> 32); }
}

// uniform scalar by the reference's wide reduction (represent.rs:18-28,80-103): (lo + hi*2^256) mod p
template <class P>
__global__ void __launch_bounds__(256) k_gen_scalars(uint64_t seed, size_t start, size_t n, uint64_t* __restrict__ out) {
  KG_SERVICE_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t lo[8], hi[8], wo[8];
  stream_words(seed, start + i, lo, hi);
  Fp<P> a = mul(limbs_from_words<P>(lo), Fp<P>::from_const(P::C_INT_TO_MONT));
  Fp<P> b = mul(limbs_from_words<P>(hi), Fp<P>::from_const(P::C_INT_HI_TO_MONT));
  to_ref(norm(add(a, b)), wo);
  store_words(out, i, wo);
}

template <class P>
__device__ __forceinline__ bool feq(const Fp<P>& a, const Fp<P>& b) { return is_zero(norm(sub<4, 1>(a, b))); }

// square root in Fq (q = 3 mod 4): a^((q+1)/4), accepted iff it squares back (bn254/src/fq.rs:121-127)
__device__ bool sqrt_field(const Fq& a, Fq& y) {
  y = pow_words(a, FqParams::E_SQRT);
  return feq(sqr(y), a);
}
// Tonelli-Shanks in Fr (bn254/src/fr.rs:165-208), returning the root with the smaller canonical integer
__device__ bool sqrt_field(const Fr& a, Fr& y) {
  using P = FrParams;
  if (is_zero(a)) { y = Fr::zero(); return true; }
  if (!feq(pow_words(a, P::E_P_MINUS_1_HALF), Fr::one())) return false;
  Fr c = Fr::from_const(P::ROOT_OF_UNITY);
  Fr tt = pow_words(a, P::E_TS_T);
  Fr r = pow_words(a, P::E_TS_T1H);
  int m = P::TS_S;
  while (!feq(tt, Fr::one())) {
    int i = 0;
    Fr x = tt;
    while (!feq(x, Fr::one())) { x = sqr(x); ++i; }
    Fr b = c;
    for (int j = 0; j < m - i - 1; ++j) b = sqr(b);
    m = i;
    c = sqr(b);
    tt = mul(tt, c);
    r = mul(r, b);
  }
  Fr nr = vred(norm(sub<4, 1>(Fr::zero(), r)));
  // compare canonical integers: mont(x*2^261, 1) = x
  Fr one_raw = Fr::zero();
  one_raw.l[0] = 1;
  Fr ri = reduce_2p(mul(r, one_raw));
  Fr ni = reduce_2p(mul(nr, one_raw));
  bool n_smaller = false;
  for (int k = 8; k >= 0; --k) {
    if (ri.l[k] != ni.l[k]) { n_smaller = ni.l[k] < ri.l[k]; break; }
  }
  y = n_smaller ? nr : r;
  return true;
}

template <class F> struct CurveB;
template <> struct CurveB<Fq> { static __device__ Fq b() { return Fq::from_const(FqParams::G1_B); } };
template <> struct CurveB<Fr> { static __device__ Fr b() { return Fr::from_const(FrParams::GRUMPKIN_B); } };

// valid curve point by try-and-increment on a seeded x (oracle/pyoracle.py base_at)
template <class F>
__global__ void __launch_bounds__(64) k_gen_bases(uint64_t seed, size_t start, size_t n, uint64_t* __restrict__ out) {
  using P = typename F::Params;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t lo[8], hi[8];
  stream_words(seed, start + i, lo, hi);
  F x = mul(limbs_from_words<P>(lo), F::from_const(P::C_INT_TO_MONT));
  F y;
  const F b = CurveB<F>::b();
  for (;;) {
    F rhs = norm(add(mul(sqr(x), x), b));
    if (sqrt_field(rhs, y) && !is_zero(y)) break;
    x = vred(norm(add(x, F::one())));
  }
  if (hi[0] & 1) y = vred(norm(sub<4, 1>(F::zero(), y)));
  uint32_t wx[8], wy[8];
  to_ref(x, wx);
  to_ref(y, wy);
  store_words(out, 2 * i, wx);
  store_words(out, 2 * i + 1, wy);
}

// ---- host half --------------------------------------------------------------------------------------
bool field_ok(int field) { return field == KG_FR || field == KG_FQ; }
// fn(P{}) with the field's parameter type: every launch of a kernel templated on it goes through here
template <class Fn>
void by_field(int field, Fn&& fn) {
  if (field == KG_FR) fn(FrParams{});
  else fn(FqParams{});
}
dim3 grid256(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// One operation against `count` vectors (strides in elements, r1cs_batch.h), the counters of ws cleared on the stream before: two launches per
// chunk of 65535 vectors, whatever count is -- for one vector grid256(m) blocks of lanes and 256 blocks of waves.  make_op(chunk): the
// operation for the chunk's vectors, its pointers offset to the chunk's first; the first chunk's first launch builds the work list, every
// later launch reads it.  then(chunk): what else the chunk needs (the product's huge rows).
template <class MakeOp, class Then>
void launch_rows(hipStream_t st, size_t m, size_t count, const RowWs& ws, MakeOp&& make_op, Then&& then) {
  for (size_t i = 0; i < r1cs_batch_chunks(count); ++i) {
    const R1csBatchChunk ch = r1cs_batch_chunk(count, i);
    const auto op = make_op(ch);
    using Op = std::remove_const_t<decltype(op)>;
    const unsigned y = (unsigned)ch.count;
    hipLaunchKernelGGL(k_rows_lane<Op>, dim3(grid256(m).x, y), dim3(256), 0, st, op, m, ws, i == 0);
    hipLaunchKernelGGL(k_rows_wave<Op>, dim3(r1cs_batch_grid_x(256, ch.count), y), dim3(256), 0, st, op, ws.list, ws.count);
    then(ch);
  }
}
template <class MakeOp>
void launch_rows(hipStream_t st, size_t m, size_t count, const RowWs& ws, MakeOp&& make_op) {
  launch_rows(st, m, count, ws, make_op, [](const R1csBatchChunk&) {});
}
CsrView view(const kg_csr* x) { return {x->d_row_ptr, x->d_col, x->d_val}; }
// a, b, c all there, with all their arrays?
bool csr3_ok(const kg_csr* a, const kg_csr* b, const kg_csr* cm) {
  for (const kg_csr* x : {a, b, cm})
    if (!x->d_row_ptr || !x->d_col || !x->d_val) return false;
  return true;
}

// u * 2^266 mod p as limbs: ten modular doublings of the ABI form u * 2^256
Limbs9 scaled(const uint64_t* h_u, bool fr) {
  Limbs9 out;
  uint64_t w64[4];
  if (fr) u_scaled_words<HostFrP>(h_u, w64);
  else u_scaled_words<HostFqP>(h_u, w64);
  const Fp<FrParams> lim = limbs_from_words<FrParams>(words8(w64).w);        // the spreading is the same for both fields
  for (int k = 0; k < 9; ++k) out.l[k] = lim.l[k];
  return out;
}

}  // namespace

extern "C" {

int kg_field_vec_op(kg_ctx* c, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  if (!c || op < 0 || op > KG_OP_TO_MONT || !field_ok(field)) return KG_ERR_BAD_ARG;
  if (n == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  const bool binary = (op == KG_OP_ADD || op == KG_OP_SUB || op == KG_OP_MUL);
  if (!a || !out || (binary && !b)) return KG_ERR_BAD_ARG;
  by_field(field, [&](auto p) { hipLaunchKernelGGL(k_vec_op<decltype(p)>, grid256(n), dim3(256), 0, c->stream, op, a, b, out, n); });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

int kg_field_vec_scale(kg_ctx* c, int field, const uint64_t* a, const uint64_t* h_s, uint64_t* out, size_t n) {
  if (!c || !h_s || !field_ok(field)) return KG_ERR_BAD_ARG;
  if (n == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  if (!a || !out) return KG_ERR_BAD_ARG;
  by_field(field, [&](auto p) { hipLaunchKernelGGL(k_vec_scale<decltype(p)>, grid256(n), dim3(256), 0, c->stream, a, words8(h_s), out, n); });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

int kg_field_powers(kg_ctx* c, int field, const uint64_t* h_start, const uint64_t* h_base, uint64_t* out, size_t n) {
  if (!c || !h_start || !h_base || !field_ok(field)) return KG_ERR_BAD_ARG;
  if (n == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  if (!out) return KG_ERR_BAD_ARG;
  const Words8 s = words8(h_start), b = words8(h_base);
  by_field(field, [&](auto p) { hipLaunchKernelGGL(k_powers<decltype(p)>, grid256(n), dim3(256), 0, c->stream, s, b, out, n); });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

int kg_field_vec_axpy(kg_ctx* c, int field, const uint64_t* a, const uint64_t* h_s, const uint64_t* b, uint64_t* out, size_t n) {
  if (!c || !h_s || !field_ok(field)) return KG_ERR_BAD_ARG;
  if (n == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  if (!a || !b || !out) return KG_ERR_BAD_ARG;
  by_field(field, [&](auto p) { hipLaunchKernelGGL(k_vec_axpy<decltype(p)>, grid256(n), dim3(256), 0, c->stream, a, words8(h_s), b, out, n); });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

int kg_field_vec_axpy_batch(kg_ctx* c, int field, const uint64_t* d_a, size_t a_stride, const uint64_t* d_s, const uint64_t* d_b, size_t b_stride,
                            uint64_t* d_out, size_t out_stride, size_t n, size_t count) {
  if (!axpy_batch_args_ok(c, field, d_a, a_stride, d_s, d_b, b_stride, d_out, out_stride, n, count)) return KG_ERR_BAD_ARG;
  if (axpy_batch_empty(n, count)) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  const size_t total = n * count;                          // (below 2^59: count * stride * 32 fits a size_t and stride >= n)
  by_field(field, [&](auto p) {
    for (size_t first = 0; first < total; first += AXPY_BATCH_LAUNCH_MAX) {
      const size_t lanes = total - first < AXPY_BATCH_LAUNCH_MAX ? total - first : AXPY_BATCH_LAUNCH_MAX;
      hipLaunchKernelGGL(k_vec_axpy_batch<decltype(p)>, grid256(lanes), dim3(256), 0, c->stream, d_a, a_stride, d_s, d_b, b_stride, d_out, out_stride, n, first,
                         total);
    }
  });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

}  // extern "C"

namespace kg {
// one matrix against `count` vectors (strides in elements, r1cs_batch.h): a memset and three launches per chunk of 65535 vectors, whatever
// count is; the first chunk's first launch builds the work list, every later launch reads it
int r1cs_prod_enqueue(kg_ctx* c, hipStream_t st, int field, const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t m,
                      const uint64_t* z, size_t z_stride, size_t count, uint64_t* out, size_t out_stride, const RowWs& ws) {
  KG_HIP(c, hipMemsetAsync(ws.count, 0, 8, st));
  by_field(field, [&](auto p) {
    using P = decltype(p);
    launch_rows(
        st, m, count, ws,
        [&](const R1csBatchChunk& ch) { return ProdOp<P>{{row_ptr, col, val}, z + ch.first * z_stride * 4, z_stride, out + ch.first * out_stride * 4, out_stride}; },
        [&](const R1csBatchChunk& ch) {
          hipLaunchKernelGGL(k_r1cs_rows_huge<P>, dim3(r1cs_batch_grid_x(64, ch.count), (unsigned)ch.count), dim3(LONG_NT), 0, st, row_ptr, col, val,
                             z + ch.first * z_stride * 4, z_stride, out + ch.first * out_stride * 4, out_stride, ws.list, ws.count, m);
        });
  });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}
}  // namespace kg

extern "C" {

int kg_r1cs_prod(kg_ctx* c, int field, const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t m, const uint64_t* z, uint64_t* out) {
  if (!c || !field_ok(field)) return KG_ERR_BAD_ARG;
  if (m == 0) return KG_OK;
  if (!row_ptr || !col || !val || !z || !out) return KG_ERR_BAD_ARG;
  KG_HIP(c, hipSetDevice(c->device));
  if (m >= ((size_t)1 << 32)) return set_err(c, KG_ERR_BAD_ARG, "more than 2^32 rows");
  KG_TRY(c->ws_vec.ensure(DevMem{c, "workspace allocation"}, RowWs::bytes(m)));
  return kg::r1cs_prod_enqueue(c, c->stream, field, row_ptr, col, val, m, z, 0, 1, out, m, RowWs(c->ws_vec.get(), m));
}

int kg_r1cs_prod_batch(kg_ctx* c, int field, const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t m, const uint64_t* z,
                       size_t z_stride, size_t count, uint64_t* out, size_t out_stride) {
  if (!r1cs_batch_args_ok(c, field, row_ptr, col, val, m, z, z_stride, count, out, out_stride)) return KG_ERR_BAD_ARG;
  if (r1cs_batch_empty(m, count)) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  KG_TRY(c->ws_vec.ensure(DevMem{c, "workspace allocation"}, RowWs::bytes(m)));
  return kg::r1cs_prod_enqueue(c, c->stream, field, row_ptr, col, val, m, z, z_stride, count, out, out_stride, RowWs(c->ws_vec.get(), m));
}

int kg_r1cs_evaluate(kg_ctx* c, const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t m, const uint64_t* z, uint64_t* out) {
  return kg_r1cs_prod(c, KG_FR, row_ptr, col, val, m, z, out);
}

}  // extern "C"

namespace {
// The cross term of one shape against `count` pairs, after the entry's argument checks: a memset, then two launches per chunk (launch_rows).
// d_u1, d_u2: a u per pair on the device, or null: us1, us2, one for every pair (DEV_U = false: both null).  Nothing is read back.
template <bool DEV_U>
int cross_enqueue(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const uint64_t* d_z1, size_t z1_stride,
                  const uint64_t* d_z2, size_t z2_stride, size_t count, const uint64_t* d_u1, const uint64_t* d_u2, const Limbs9& us1, const Limbs9& us2,
                  uint64_t* d_out, size_t out_stride) {
  KG_TRY(c->ws_vec.ensure(DevMem{c, "workspace allocation"}, RowWs::bytes(m)));
  const RowWs ws(c->ws_vec.get(), m);
  KG_HIP(c, hipMemsetAsync(ws.count, 0, 8, c->stream));
  by_field(field, [&](auto p) {
    launch_rows(c->stream, m, count, ws, [&](const R1csBatchChunk& ch) {
      return CrossOp<decltype(p), DEV_U>{{view(a), view(b), view(cm)}, d_z1 + ch.first * z1_stride * 4, z1_stride, d_z2 + ch.first * z2_stride * 4, z2_stride,
                                         d_u1 ? d_u1 + ch.first * 4 : nullptr, d_u2 ? d_u2 + ch.first * 4 : nullptr, us1, us2, d_out + ch.first * out_stride * 4, out_stride};
    });
  });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}
// The check of one shape against `count` vectors read through the source Z, after the entry's argument checks and with the work space there:
// one initialising launch, then two launches per chunk (launch_rows).  d_u: a u per vector on the device, or null: `us`, one for every
// vector.  Nothing is read back.
template <class Z>
int check_enqueue(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const RowWs& ws, const Z& z, size_t count,
                  const uint64_t* d_u, const Limbs9& us, const uint64_t* d_e, size_t e_stride, uint8_t* d_status, size_t status_stride, uint32_t* d_summary) {
  hipLaunchKernelGGL(k_check_batch_init, grid256(count), dim3(256), 0, c->stream, d_summary, count, (uint32_t)m, ws.count);
  by_field(field, [&](auto p) {
    launch_rows(c->stream, m, count, ws, [&](const R1csBatchChunk& ch) {
      return CheckOp<decltype(p), Z>{{view(a), view(b), view(cm)}, z.from(ch.first), d_u ? d_u + ch.first * 4 : nullptr, us,
                                     d_e ? d_e + ch.first * e_stride * 4 : nullptr, e_stride, d_status ? d_status + ch.first * status_stride : nullptr,
                                     status_stride, d_summary + 2 * ch.first};
    });
  });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}
// u = 1 in the factor form, for the calls without a u of their own
Limbs9 scaled_one(int field) { return scaled(field == KG_FR ? HostFrP::ONE : HostFqP::ONE, field == KG_FR); }
// the two batched checks after their argument checks
template <class Z>
int check_batch_enqueue(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const Z& z, size_t count, const uint64_t* d_u,
                        const uint64_t* d_e, size_t e_stride, uint8_t* d_status, size_t status_stride, uint32_t* d_summary) {
  KG_HIP(c, hipSetDevice(c->device));
  if (m == 0) {                                            // no row, no list: the pairs alone, (0, 0)
    hipLaunchKernelGGL(k_check_batch_init, grid256(count), dim3(256), 0, c->stream, d_summary, count, 0u, (uint32_t*)nullptr);
    KG_HIP(c, hipGetLastError());
    return KG_OK;
  }
  KG_TRY(c->ws_vec.ensure(DevMem{c, "workspace allocation"}, RowWs::bytes(m)));
  return check_enqueue(c, field, a, b, cm, m, RowWs(c->ws_vec.get(), m), z, count, d_u, scaled_one(field), d_e, e_stride, d_status, status_stride, d_summary);
}
}  // namespace

extern "C" {

int kg_nova_cross_term(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const uint64_t* d_z1,
                       const uint64_t* d_z2, const uint64_t* h_u1, const uint64_t* h_u2, uint64_t* d_out) {
  if (!c || !field_ok(field) || !a || !b || !cm || !h_u1 || !h_u2) return KG_ERR_BAD_ARG;
  if (m == 0) return KG_OK;
  if (!d_z1 || !d_z2 || !d_out || !csr3_ok(a, b, cm)) return KG_ERR_BAD_ARG;
  KG_HIP(c, hipSetDevice(c->device));
  const Limbs9 u1 = scaled(h_u1, field == KG_FR), u2 = scaled(h_u2, field == KG_FR);
  if (m >= ((size_t)1 << 32)) return set_err(c, KG_ERR_BAD_ARG, "more than 2^32 rows");
  return cross_enqueue<false>(c, field, a, b, cm, m, d_z1, 0, d_z2, 0, 1, nullptr, nullptr, u1, u2, d_out, m);
}

int kg_nova_cross_term_batch(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const uint64_t* d_z1, size_t z1_stride,
                             const uint64_t* d_z2, size_t z2_stride, size_t count, const uint64_t* d_u1, const uint64_t* d_u2, uint64_t* d_out,
                             size_t out_stride) {
  if (!nova_cross_batch_args_ok(c, field, a, b, cm, m, d_z1, z1_stride, d_z2, z2_stride, count, d_out, out_stride)) return KG_ERR_BAD_ARG;
  if (r1cs_batch_empty(m, count)) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  const Limbs9 one = scaled_one(field);
  return cross_enqueue<true>(c, field, a, b, cm, m, d_z1, z1_stride, d_z2, z2_stride, count, d_u1, d_u2, one, one, d_out, out_stride);
}

int kg_r1cs_check(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const uint64_t* d_z, const uint64_t* h_u,
                  const uint64_t* d_e, uint8_t* d_status, size_t* out_bad, size_t* out_first_bad) {
  if (!c || !field_ok(field) || !a || !b || !cm) return KG_ERR_BAD_ARG;
  if (m >= ((size_t)1 << 32)) return set_err(c, KG_ERR_BAD_ARG, "more than 2^32 rows");
  if (m == 0) {
    if (out_bad) *out_bad = 0;
    if (out_first_bad) *out_first_bad = 0;
    return KG_OK;
  }
  if (!d_z || !csr3_ok(a, b, cm)) return KG_ERR_BAD_ARG;
  KG_HIP(c, hipSetDevice(c->device));
  const Limbs9 us = h_u ? scaled(h_u, field == KG_FR) : scaled_one(field);       // no u: the plain relation, u = 1
  KG_TRY(c->ws_vec.ensure(DevMem{c, "workspace allocation"}, RowWs::bytes(m)));
  const RowWs ws(c->ws_vec.get(), m);
  KG_TRY(check_enqueue(c, field, a, b, cm, m, ws, ZStrided{d_z, 0}, 1, nullptr, us, d_e, 0, d_status, 0, ws.summary));
  return summary_read(c, ws.summary, out_bad, out_first_bad);
}

int kg_r1cs_check_batch(kg_ctx* c, int field, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, const uint64_t* d_z, size_t z_stride, size_t count,
                        const uint64_t* d_u, const uint64_t* d_e, size_t e_stride, uint8_t* d_status, size_t status_stride, uint32_t* d_summary) {
  if (!r1cs_check_batch_args_ok(c, field, a, b, cm, m, d_z, z_stride, count, d_e, e_stride, d_status, status_stride, d_summary)) return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  return check_batch_enqueue(c, field, a, b, cm, m, ZStrided{d_z, z_stride}, count, d_u, d_e, e_stride, d_status, status_stride, d_summary);
}

int kg_groth16_witness_check_batch(kg_ctx* c, const kg_csr* a, const kg_csr* b, const kg_csr* cm, size_t m, size_t l, size_t m_l_1, const uint64_t* d_x,
                                   size_t x_stride, const uint64_t* d_w, size_t w_stride, size_t count, uint8_t* d_status, size_t status_stride,
                                   uint32_t* d_summary) {
  if (!g16_witness_check_batch_args_ok(c, a, b, cm, m, l, m_l_1, d_x, x_stride, d_w, w_stride, count, d_status, status_stride, d_summary)) return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  return check_batch_enqueue(c, KG_FR, a, b, cm, m, ZSplitStrided{d_x, x_stride, d_w, w_stride, l}, count, nullptr, nullptr, 0, d_status, status_stride, d_summary);
}

int kg_gen_scalars(kg_ctx* c, int field, uint64_t seed, size_t start, size_t n, uint64_t* out) {
  if (!c || !field_ok(field)) return KG_ERR_BAD_ARG;
  if (n == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  if (!out) return KG_ERR_BAD_ARG;
  by_field(field, [&](auto p) { hipLaunchKernelGGL(k_gen_scalars<decltype(p)>, grid256(n), dim3(256), 0, c->stream, seed, start, n, out); });
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

int kg_gen_bases(kg_ctx* c, int curve, uint64_t seed, size_t start, size_t n, uint64_t* out) {
  if (!c || (curve != KG_G1 && curve != KG_GRUMPKIN)) return KG_ERR_BAD_ARG;
  if (n == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  if (!out) return KG_ERR_BAD_ARG;
  dim3 grid((unsigned)((n + 63) / 64));
  if (curve == KG_G1) hipLaunchKernelGGL(k_gen_bases<Fq>, grid, dim3(64), 0, c->stream, seed, start, n, out);
  else hipLaunchKernelGGL(k_gen_bases<Fr>, grid, dim3(64), 0, c->stream, seed, start, n, out);
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

}  // extern "C"
