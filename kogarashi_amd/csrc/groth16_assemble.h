// groth16_assemble.h -- the assembly of a Groth16 proof (groth16/src/prover.rs:75-92) as templates over the field type.  With the five
// sums Sa, Sb1, Sb2, Sl, Sh of a proof (the MSMs against a, b_g1, b_g2, l and h):
//   A = r delta1 + alpha + Sa
//   B = s delta2 + beta2 + Sb2
//   C = r s delta1 + (s alpha + r beta1) + (s Sa + r Sb1) + Sh + Sl
// Every scalar multiple is ONE chain, g16_mul2(P, k1, Q, k2) = k1 P + k2 Q, most significant bit first over the canonical integers of
// the scalars; a chain's role says which points and scalars it takes, so the lanes of the batched prover (groth16_batch.hip: one lane per
// proof and chain) differ in data only:
//   role 0  (delta1, r,   -,     0)        role 2  (alpha, s, beta1, r)        role 4, in Fq2  (delta2, s, -, 0)
//   role 1  (delta1, r s, -,     0)        role 3  (Sa,    s, Sb1,   r)
// KG_HD: tests/host/g16_batch_host.cpp compiles the chain and the formulas for the host over the device's field type, over the
// bound-tracking type (fp29_checked.h) and over the host's own (host_fp.h).
#pragma once
#include "curve.h"

namespace kg {

enum { G16_ROLE_R_DELTA = 0, G16_ROLE_RS_DELTA = 1, G16_ROLE_VK = 2, G16_ROLE_SUMS = 3, G16_ROLE_G2 = 4 };

// The chain: per bit one doubling and -- unless both bits are 0 -- ONE addition of the operand the two bits select:
// ops(1) = P, ops(2) = Q, ops(3) = P + Q.  Where the operands live is the caller's business (the kernels keep them in LDS, one column per
// lane, so that the selection is an address and the chain holds one operand in registers, not three).
template <class F, class Ops>
KG_HD XYZZ<F> g16_mul2_ops(const Ops& ops, const uint32_t k1[8], const uint32_t k2[8]) {
  XYZZ<F> acc = XYZZ<F>::identity();
  for (int b = 255; b >= 0; --b) {
    acc = double_xyzz(acc);                               // (the identity doubles to itself: leading zero bits cost nothing)
    const int sel = (int)((k1[b >> 5] >> (b & 31)) & 1) | (int)(((k2[b >> 5] >> (b & 31)) & 1) << 1);
    if (sel) acc = add_xyzz(acc, ops(sel));
  }
  return acc;
}

// k1 P + k2 Q with the three operands in an array of the caller's frame
template <class F>
struct G16ArrayOps {
  XYZZ<F> t[3];
  KG_HD const XYZZ<F>& operator()(int sel) const { return t[sel - 1]; }
};
template <class F>
KG_HD XYZZ<F> g16_mul2(const XYZZ<F>& p, const uint32_t k1[8], const XYZZ<F>& q, const uint32_t k2[8]) {
  const G16ArrayOps<F> ops{{p, q, add_xyzz(p, q)}};
  return g16_mul2_ops<F>(ops, k1, k2);
}

// P + k Q -- the instance fold of a Nova step (nova/src/relaxed_r1cs/instance.rs:81-101), points_fold.hip -- is the chain with k1 = 1: bit 0
// of k1 brings P in at the last step.  k_ref: the scalar in the ABI's Montgomery form over the curve's scalar field (parameters SP).
template <class F, class SP, class Ops>
KG_HD XYZZ<F> muladd_chain_ops(const Ops& ops, const uint32_t k_ref[8]) {
  uint32_t ki[8];
  ref_to_int<SP>(k_ref, ki);
  const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  return g16_mul2_ops<F>(ops, one, ki);
}

// The scalars of a role as canonical integers, from r and s in the ABI's Montgomery form; r s is one field product.  Every role computes
// all of them and selects.
KG_HD void g16_chain_scalars(int role, const uint32_t r_ref[8], const uint32_t s_ref[8], uint32_t k1[8], uint32_t k2[8]) {
  uint32_t ri[8], si[8], rs_ref[8], rsi[8];
  ref_to_int<FrParams>(r_ref, ri);
  ref_to_int<FrParams>(s_ref, si);
  to_ref(mul(from_ref<FrParams>(r_ref), from_ref<FrParams>(s_ref)), rs_ref);
  ref_to_int<FrParams>(rs_ref, rsi);
  const bool two = role == G16_ROLE_VK || role == G16_ROLE_SUMS;
  for (int i = 0; i < 8; ++i) {
    k1[i] = role == G16_ROLE_R_DELTA ? ri[i] : (role == G16_ROLE_RS_DELTA ? rsi[i] : si[i]);
    k2[i] = two ? ri[i] : 0u;
  }
}

// A = r delta1 + alpha + Sa, and B likewise in G2 (prover.rs:75-76, 81, 88)
template <class F>
KG_HD XYZZ<F> g16_point_ab(const XYZZ<F>& k_delta, const XYZZ<F>& vk, const XYZZ<F>& sum) { return add_xyzz(add_xyzz(k_delta, vk), sum); }
// C = r s delta1 + (s alpha + r beta1) + (s Sa + r Sb1) + Sl + Sh (prover.rs:77, 83, 90, 92)
template <class F>
KG_HD XYZZ<F> g16_point_c(const XYZZ<F>& rs_delta, const XYZZ<F>& sa_rb, const XYZZ<F>& sa_rb1, const XYZZ<F>& sl, const XYZZ<F>& sh) {
  return add_xyzz(add_xyzz(add_xyzz(add_xyzz(rs_delta, sa_rb), sa_rb1), sl), sh);
}

}  // namespace kg
