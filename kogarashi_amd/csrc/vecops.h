// vecops.h -- the lazy arithmetic of the vector kernels (vec.hip) as templates over the field type, so that the host
// bound checker (tests/host/hosttest.cpp, F = FpChecked) proves the same instruction sequences the device runs.
//
// Values cross memory in the ABI's Montgomery domain (x * 2^256).  A raw load times a constant in internal form (c * 2^261)
// Montgomery-multiplies to x * c * 2^256 (fp29.h: mul divides by 2^261); a raw load times a raw load gives x y 2^251, and the
// sparse products below stay in that domain until a constant the next multiplication needs anyway takes them out of it.
#pragma once
#include "fp29.h"
#include "host_fp.h"

namespace kg {

// one term of a sparse row product (zkstd/src/matrix/row.rs:43-51): sum + z * v with BOTH factors raw (the ABI words as
// limbs, any 256-bit value): the term is z * v * 2^512 / 2^261, i.e. the sums live in the "raw product" domain x * 2^251
template <class F>
KG_HD F dot_step(const F& sum, const F& z_raw, const F& v_raw) { return vred(norm(add(sum, mul(z_raw, v_raw)))); }
// two partial sums of one row
template <class F>
KG_HD F dot_merge(const F& a, const F& b) { return vred(norm(add(a, b))); }

// one element of a Nova fold (nova/src/relaxed_r1cs/witness.rs:56-70): a + s * b with a and b raw (the ABI words as limbs, any 256-bit
// value) and s in internal form (from_ref of its ABI words: s * 2^261, below 2p): raw(b) * internal(s) stays in the ABI's Montgomery
// domain, like raw(a).  One product, a lazy sum, one value reduction; the caller canonicalises (reduce_2p).  Both axpy kernels run this body: the single
// call's (a scalar by value) and the batch's (a scalar per vector, read on the device).
template <class F>
KG_HD F axpy_step(const F& a_raw, const F& b_raw, const F& s) { return vred(norm(add(a_raw, mul(b_raw, s)))); }

// Nova's cross term for one constraint row (nova/src/prover.rs:81-89):
//   AZ1 * BZ2 + AZ2 * BZ1 - u1 * CZ2 - u2 * CZ1
// az*, bz*, cz*: row sums as dot_step / dot_merge leave them (x * 2^251, below 1.06p).  u1s, u2s: u * 2^266 (the ABI form
// times 2^10; C_XT_U does it on the device, ten doublings on the host), so that (c * 2^251)(u * 2^266) / 2^261 = c u 2^256.
// had_const: 2^276 (P::C_XT_HAD): (a * 2^251)(b * 2^251) / 2^261 = a b 2^241, times 2^276 / 2^261 = a b 2^256.
// Result: ABI domain, normalised, below 2p (the caller canonicalises).
template <class F>
KG_HD F cross_term_row(const F& az1, const F& az2, const F& bz1, const F& bz2, const F& cz1, const F& cz2, const F& u1s, const F& u2s,
                       const F& had_const) {
  const F had = mul(mul2add(az1, bz2, az2, bz1), had_const);
  const F c1 = mul(cz2, u1s);
  const F c2 = mul(cz1, u2s);
  return vred(norm(sub<8, 1>(norm(sub<4, 1>(had, c1)), c2)));
}

// The residual of one constraint row of the (relaxed) R1CS relation (nova/src/relaxed_r1cs.rs:81-114 is_sat_relaxed; with u = 1, E = 0
// zkstd/src/r1cs.rs:62-77 is_sat):   (A z)_i (B z)_i - u (C z)_i - E_i,   in the ABI domain (times 2^256).
// az, bz, cz: row sums as dot_step / dot_merge leave them (x * 2^251, normalised, below 1.06p; zero() for an empty row).
// us: u * 2^266, normalised, below 2p (the kernel gets the canonical value from ten host-side doublings of the ABI form; the Montgomery
//     one doubled ten times when the caller has no u).  e_raw: E_i as it lies in memory (the ABI words as limbs: any 256-bit value,
//     below 5.4p, limbs normalised by the unpacking); zero() when the caller has no E.  had_const: 2^276 (P::C_XT_HAD).
// Bounds: the two products are normalised and below 1.01p, so 4p dominates the first subtrahend and 8p the raw word (sub<4, 1>, sub<8, 1>:
// limbs up to 2^29 - 1, top limb below the fat constant's); the lazy value had + 4p - c + 8p - e lies in (5.5p, 13.1p), its top limb
// below 2^27 after the carries, which is what vred accepts.  Result: normalised, below 1.06p.
template <class F>
KG_HD F sat_residual_row(const F& az, const F& bz, const F& cz, const F& us, const F& e_raw, const F& had_const) {
  const F had = mul(mul(az, bz), had_const);
  const F cu = mul(cz, us);
  return vred(norm(sub<8, 1>(norm(sub<4, 1>(had, cu)), e_raw)));
}
// u as it lies in memory (the ABI words as limbs, u * 2^256, any 256-bit value) -> the factor form `us` of sat_residual_row, u * 2^266: one
// product with xt_u = 2^271 (P::C_XT_U).  The batched check does this on the device, a u per vector; the single call gets the same residue from
// ten host-side doublings (vec.hip scaled()).  Result: normalised, below 1.01p -- a representative of scaled()'s canonical value.
template <class F>
KG_HD F u_factor(const F& u_raw, const F& xt_u) { return mul(u_raw, xt_u); }

// The host's way to the same factor (vec.hip scaled(): kg_r1cs_check, kg_nova_cross_term): u * 2^266 mod p, canonical, as 4 x u64 -- ten
// modular doublings of the ABI form.  HostP: HostFrP or HostFqP.
template <class HostP>
inline void u_scaled_words(const uint64_t* h_u, uint64_t out[4]) {
  HostFp<HostP> x = HostFp<HostP>::from_words(h_u);
  for (int i = 0; i < 10; ++i) x = dbl(x);
  x.to_words(out);
}

// Is a residual as sat_residual_row leaves it zero in the field?  The value is the canonical residue or that plus p (vred's quotient
// estimate may be one short), never more: a row that holds arrives as 0 or as p.  BOTH occur -- the lazy value of a satisfied row is k p
// with 6 <= k <= 13 and vred takes off k p or (k - 1) p, decided by the top limb alone (a row with no entries and E = 0 is the lazy
// value 12p: limbs of the two fat constants, nothing else).  So the test compares with both representatives, which is what canonicalising (reduce_2p: p -> 0) and
// comparing with zero comes to, without the subtraction.  Inputs outside [0, 2p) are a bound violation (FpChecked aborts on them).
template <class F>
KG_HD bool is_zero_mod_p(const F& residual) { return is_zero_2p(residual); }

}  // namespace kg
