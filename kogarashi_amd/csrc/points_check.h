// points_check.h -- per-point validation predicates of kg_points_check (points.hip): canonical coordinate words, the curve equation of the
// three curves of the path, and the order-r subgroup of the BN254 twist.  Everything is KG_HD and a template over the field type, so that the
// kernels and the host twin of tests/host/points_check_host.cpp (plain types, and the bound-tracking FpChecked shadow) run the same code.
//
// Semantics (include/kogarashi_amd.h, kg_points_check): a finite point is NON_CANONICAL when a coordinate word value is >= p (an integer
// comparison on the words, nothing else is looked at), else OFF_CURVE when y^2 != x^3 + b, else -- G2 with the subgroup check asked for --
// NOT_IN_SUBGROUP when [r]P != O.  The reference's predicates are Group::is_on_curve (zkstd/src/macros/curve/weierstrass/group.rs:59-65) and
// G2Affine::is_torsion_free (bn254/src/g2.rs:26); the latter tests psi(P) == [x]P, the BLS12-381 criterion, which rejects the BN254 generator
// for either sign of x, so it is the call site this replaces and not the specification: the specification is [r]P = O.
//
// The subgroup test.  psi = twist o Frobenius o untwist, psi(x, y) = (conj(x) GX, conj(y) GY) (psi_consts.h), is an endomorphism of the
// whole twist E'(Fq2) -- it is defined on every on-curve point, in the subgroup or not -- that satisfies psi^2 - t psi + q = 0 and acts on the
// order-r subgroup as multiplication by q mod r.  With q, r, t polynomials in the BN parameter x, the test evaluated for [r]P = O is
//     [x + 1]P + psi([x]P) + psi^2([x]P) = psi^3([2x]P)
// (it holds on the subgroup; that it fails off it is checked against [r]P = O with Python integers on random twist points, their [h2] images,
// points of order 10069 and 5864401 and mixed sums: tests/test_points_check_host.py, tests/test_gpu_points_check.py).  Evaluated Horner-wise as psi(Q + psi(Q - psi(2Q))) + Q + P = O with
// Q = [x]P: 62 doublings and 27 mixed additions for Q (x has 63 bits, 28 set), one more doubling, three psi (two Fq2 products each) and
// four additions -- about 95 point operations where the plain [r]P chain takes 353.  x is public: the loop has a fixed trip count and its
// branch on the bit of x is uniform; the data-dependent branches are the exceptional cases inside the complete formulas of curve.h
// (identity operand, equal x), which low-order inputs do reach.  No on-curve twist point has y = 0 (#E'(Fq2) = r (2q - r) is odd), so
// double_xyzz needs no such case.
#pragma once
#include <type_traits>
#include "curve.h"
#include "psi_consts.h"

namespace kg {
namespace pts {

constexpr uint8_t ST_NON_CANONICAL = 1, ST_OFF_CURVE = 2, ST_NOT_IN_SUBGROUP = 4;      // = KG_PT_* of the public header (points.hip asserts it)

// integer value of the 8 words < p
template <class P>
KG_HD bool words_below_p(const uint32_t* w) {
  uint32_t pw[8];
  words_from_limbs(Fp<P>::from_const(P::P), pw);
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)w[i] - pw[i] - borrow;
    borrow = (uint32_t)(d >> 63);
  }
  return borrow != 0;
}

// ABI words -> a base-field element of type E (Fp<P>; the host test adds FpChecked<P>)
template <class E> struct Elem;
template <class P> struct Elem<Fp<P>> {
  static KG_HD Fp<P> from_ref_words(const uint32_t* w) { return from_ref<P>(w); }      // any 256-bit input; normalised, < 2p
};

// a coordinate: NW ABI words, the canonicity test, the conversion and the curve's b
template <class F> struct Coord {
  using P = typename F::Params;
  static constexpr int NW = 8;
  static KG_HD bool canonical(const uint32_t* w) { return words_below_p<P>(w); }
  static KG_HD F load(const uint32_t* w) { return Elem<F>::from_ref_words(w); }
  static KG_HD F b() {
    if constexpr (std::is_same<P, FqParams>::value) return F::from_const(FqParams::G1_B);          // y^2 = x^3 + 3
    else return F::from_const(FrParams::GRUMPKIN_B);                                              // y^2 = x^3 - 17
  }
};
template <class E> struct Coord<Fp2<E>> {
  static constexpr int NW = 16;
  static KG_HD bool canonical(const uint32_t* w) { return Coord<E>::canonical(w) && Coord<E>::canonical(w + 8); }
  static KG_HD Fp2<E> load(const uint32_t* w) { return {Coord<E>::load(w), Coord<E>::load(w + 8)}; }
  static KG_HD Fp2<E> b() { return {E::from_const(FqParams::G2_B_C0), E::from_const(FqParams::G2_B_C1)}; }   // 3 / (9 + u)
};

// y^2 == x^3 + b for coordinates as Coord::load returns them (normalised, < 2p)
template <class F>
KG_HD bool on_curve(const F& x, const F& y) {
  const F rhs = norm(add(mul(sqr(x), x), Coord<F>::b()));       // < 3.1p
  return is_zero(norm(sub<8, 1>(sqr(y), rhs)));
}

// words of one finite point (x | y) -> its curve status, the converted point in `a`
template <class F>
KG_HD uint8_t curve_status(const uint32_t* w, Affine<F>& a) {
  constexpr int NW = Coord<F>::NW;
  const bool canon = Coord<F>::canonical(w) && Coord<F>::canonical(w + NW);
  a.x = Coord<F>::load(w);
  a.y = Coord<F>::load(w + NW);
  const bool on = on_curve(a.x, a.y);           // evaluated for every lane: no divergence on the common path
  return !canon ? ST_NON_CANONICAL : (on ? (uint8_t)0 : ST_OFF_CURVE);
}

template <class E>
KG_HD Fp2<E> conj(const Fp2<E>& a) { return {a.c0, vred(norm(sub<4, 1>(E::zero(), a.c1)))}; }

// psi on XYZZ coordinates: x = X / ZZ, y = Y / ZZZ, so all four coordinates are conjugated and X, Y take the constants
template <class E>
KG_HD XYZZ<Fp2<E>> psi(const XYZZ<Fp2<E>>& p) {
  if (is_identity(p)) return p;
  const Fp2<E> gx = {E::from_const(PsiConsts::GX_C0), E::from_const(PsiConsts::GX_C1)};
  const Fp2<E> gy = {E::from_const(PsiConsts::GY_C0), E::from_const(PsiConsts::GY_C1)};
  return {mul(conj(p.x), gx), mul(conj(p.y), gy), conj(p.zz), conj(p.zzz)};
}

// [x]P, x the BN parameter: left-to-right double-and-add over the constant bits of x (fixed trip count)
template <class E>
KG_HD XYZZ<Fp2<E>> mul_bn_x(const Affine<Fp2<E>>& P) {
  XYZZ<Fp2<E>> q = from_affine(P);
#pragma unroll 1
  for (int i = PsiConsts::BN_X_BITS - 2; i >= 0; --i) {
    q = double_xyzz(q);
    if ((PsiConsts::BN_X >> i) & 1) q = add_mixed(q, P);
  }
  return q;
}

// [r]P == O for an on-curve point P of the twist
template <class E>
KG_HD bool g2_in_subgroup(const Affine<Fp2<E>>& P) {
  const XYZZ<Fp2<E>> q = mul_bn_x(P);
  XYZZ<Fp2<E>> t = psi(double_xyzz(q));
  t = psi(add_xyzz(q, neg_xyzz(t)));
  t = psi(add_xyzz(q, t));
  t = add_mixed(add_xyzz(t, q), P);
  return is_identity(t);
}

// G1 and Grumpkin have cofactor 1: every on-curve point is in the group
template <class F> struct Subgroup { static KG_HD bool has(const Affine<F>&) { return true; } };
template <class E> struct Subgroup<Fp2<E>> { static KG_HD bool has(const Affine<Fp2<E>>& a) { return g2_in_subgroup(a); } };

// the whole decision for one point: w = its 2 * NW ABI words, identity = its flag (an identity's coordinates are not examined)
template <class F, bool SUB>
KG_HD uint8_t point_status(const uint32_t* w, bool identity) {
  if (identity) return 0;
  Affine<F> a;
  uint8_t st = curve_status<F>(w, a);
  if constexpr (SUB) {
    if (st == 0 && !Subgroup<F>::has(a)) st = ST_NOT_IN_SUBGROUP;      // non-canonical and off-curve points skip the chain
  }
  return st;
}

}  // namespace pts
}  // namespace kg
