// arith_cases.h -- the per-element cases of the arithmetic tests, written once as host/device templates: tests/host/hosttest.cpp runs them on the
// CPU (plain types and the bound-tracking FpChecked shadow), tests/device/devprobe.hip runs THE SAME LINES in test kernels on the GPU, where
// the column sums of fp29.h are inline-assembly chains and not the C loop of the host build.  Every case calls a product template; none restates one.
// Test infrastructure only.
#pragma once
#include <cstdint>
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/fp_inv.h"
#include "../../kogarashi_amd/csrc/curve.h"
#include "../../kogarashi_amd/csrc/msm_digits.h"

namespace kgcase {
using namespace kg;

// ---- ABI-form words <-> field type (plain here; hosttest.cpp adds the checked type) ---------------------------------------------------------
template <class F> struct Conv;
template <class P> struct Conv<Fp<P>> {
  static KG_HD Fp<P> in(const uint32_t* w) { return from_ref<P>(w); }
  static KG_HD void out(const Fp<P>& a, uint32_t* w) { to_ref(a, w); }
  static constexpr int W = 8;
};
template <class F> struct Conv<Fp2<F>> {
  static KG_HD Fp2<F> in(const uint32_t* w) { return {Conv<F>::in(w), Conv<F>::in(w + 8)}; }
  static KG_HD void out(const Fp2<F>& a, uint32_t* w) { Conv<F>::out(a.c0, w); Conv<F>::out(a.c1, w + 8); }
  static constexpr int W = 16;
};

template <class F> KG_HD F xsub(const F& a, const F& b) { return norm(sub<4, 1>(a, b)); }

// op: 0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 dbl, 6 inv, 7 (a*b+a*a) via lazy chain, 8 identity round trip, 9 inv by binary GCD
// a, b, o: one element each in the ABI form (Conv<F>::W words)
template <class F>
KG_HD void field_case(int op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  F x = Conv<F>::in(a), y = Conv<F>::in(b), r = x;
  switch (op) {
    case 0: r = mul(x, y); break;
    case 1: r = sqr(x); break;
    case 2: r = norm(add(x, y)); break;
    case 3: r = xsub(x, y); break;
    case 4: r = xsub(F::zero(), x); break;
    case 5: r = norm(dbl(x)); break;
    case 6: r = inv(x); break;
    case 7: r = mul(norm(add(mul(x, y), sqr(x))), F::one()); break;
    case 8: r = x; break;
    case 9: r = inv_fast(x); break;          // binary-GCD inversion (fp_inv.h)
  }
  Conv<F>::out(r, o);
}

// ---- raw limbs: 9 x uint32 taken as they are, no domain conversion --------------------------------------------------------------------------
// Raw<F>: how an operand enters the field type.  bnd = {limb bound, top-limb bound, K} of the operand's class (value < K p): the plain type
// ignores it, the checked type (hosttest.cpp) wraps the limbs with it, so an operand outside a primitive's precondition aborts on the CPU.
template <class F> struct Raw;
template <class P> struct Raw<Fp<P>> {
  static KG_HD Fp<P> limbs(const uint32_t* l, const double*) {
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = l[i];
    return r;
  }
  static KG_HD const Fp<P>& plain(const Fp<P>& a) { return a; }
  static KG_HD Fp<P> words(const uint32_t* w) { return limbs_from_words<P>(w); }
  static KG_HD Fp<P> from_ref(const uint32_t* w) { return kg::from_ref<P>(w); }
  static KG_HD Fp<P> from_int(const uint32_t* w) { return kg::from_int<P>(w); }
  static KG_HD void to_ref(const Fp<P>& a, uint32_t* w) { kg::to_ref(a, w); }
};

constexpr int RAW_OUT = 18;      // words of output per element: 9 limbs, 8 words, one flag, or the 18 limbs of an FpConst
enum RawOp {
  R_MUL = 0, R_SQR, R_MUL2ADD, R_MUL2SUB, R_MUL2PM_POS, R_MUL2PM_NEG, R_MULC, R_ADD, R_DBL, R_NORM, R_VRED, R_REDUCE_2P, R_REDUCE,
  R_IS_ZERO_2P, R_IS_ZERO, R_SAME_LIMBS, R_LIMBS_FROM_WORDS, R_WORDS_FROM_LIMBS, R_FROM_REF, R_TO_REF, R_REF_TO_INT, R_INT_TO_REF, R_FROM_INT,
  R_MAKE_CONST,
  R_SUB_2_1 = 30, R_SUB_3_1, R_SUB_4_1, R_SUB_8_1, R_SUB_16_1, R_SUB_32_1, R_SUB_4_3, R_SUB_8_3, R_SUB_16_3, R_SUB_32_3
};

// a, b, c, d: 9 limbs each (ops on words read the first 8 of a); k: the 18 limbs {w, q} of an FpConst (R_MULC); bnd: 4 x 3 bounds or null
template <class F>
KG_HD void raw_case(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, const uint32_t* k, const double* bnd,
                    uint32_t* out) {
  using P = typename F::Params;
  using R = Raw<F>;
  for (int i = 0; i < RAW_OUT; ++i) out[i] = 0;
  const double* ba = bnd; const double* bb = bnd ? bnd + 3 : nullptr; const double* bc = bnd ? bnd + 6 : nullptr; const double* bd = bnd ? bnd + 9 : nullptr;
  F r = F::zero();
  bool limbs_out = true;
  switch (op) {
    case R_MUL: r = mul(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SQR: r = sqr(R::limbs(a, ba)); break;
    case R_MUL2ADD: r = mul2add(R::limbs(a, ba), R::limbs(b, bb), R::limbs(c, bc), R::limbs(d, bd)); break;
    case R_MUL2SUB: r = mul2sub(R::limbs(a, ba), R::limbs(b, bb), R::limbs(c, bc), R::limbs(d, bd)); break;
    case R_MUL2PM_POS: r = mul2pm(R::limbs(a, ba), R::limbs(b, bb), R::limbs(c, bc), R::limbs(d, bd), false); break;
    case R_MUL2PM_NEG: r = mul2pm(R::limbs(a, ba), R::limbs(b, bb), R::limbs(c, bc), R::limbs(d, bd), true); break;
    case R_MULC: {
      FpConst<P> kc;
      for (int i = 0; i < 9; ++i) { kc.w[i] = k[i]; kc.q[i] = k[9 + i]; }
      r = mulc(R::limbs(a, ba), kc);
      break;
    }
    case R_ADD: r = add(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_DBL: r = dbl(R::limbs(a, ba)); break;
    case R_NORM: r = norm(R::limbs(a, ba)); break;
    case R_VRED: r = vred(R::limbs(a, ba)); break;
    case R_REDUCE_2P: r = reduce_2p(R::limbs(a, ba)); break;
    case R_REDUCE: r = reduce(R::limbs(a, ba)); break;
    case R_IS_ZERO_2P: out[0] = is_zero_2p(R::limbs(a, ba)) ? 1u : 0u; limbs_out = false; break;
    case R_IS_ZERO: out[0] = is_zero(R::limbs(a, ba)) ? 1u : 0u; limbs_out = false; break;
    case R_SAME_LIMBS: out[0] = same_limbs(R::plain(R::limbs(a, ba)), R::plain(R::limbs(b, bb))) ? 1u : 0u; limbs_out = false; break;
    case R_LIMBS_FROM_WORDS: r = R::words(a); break;
    case R_WORDS_FROM_LIMBS: words_from_limbs(R::plain(R::limbs(a, ba)), out); limbs_out = false; break;
    case R_FROM_REF: r = R::from_ref(a); break;
    case R_TO_REF: R::to_ref(R::limbs(a, ba), out); limbs_out = false; break;
    case R_REF_TO_INT: ref_to_int<P>(a, out); limbs_out = false; break;
    case R_INT_TO_REF: int_to_ref<P>(a, out); limbs_out = false; break;
    case R_FROM_INT: r = R::from_int(a); break;
    case R_MAKE_CONST: {
      const FpConst<P> kc = make_const(R::plain(R::limbs(a, ba)));
      for (int i = 0; i < 9; ++i) { out[i] = kc.w[i]; out[9 + i] = kc.q[i]; }
      limbs_out = false;
      break;
    }
    case R_SUB_2_1: r = sub<2, 1>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_3_1: r = sub<3, 1>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_4_1: r = sub<4, 1>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_8_1: r = sub<8, 1>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_16_1: r = sub<16, 1>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_32_1: r = sub<32, 1>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_4_3: r = sub<4, 3>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_8_3: r = sub<8, 3>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_16_3: r = sub<16, 3>(R::limbs(a, ba), R::limbs(b, bb)); break;
    case R_SUB_32_3: r = sub<32, 3>(R::limbs(a, ba), R::limbs(b, bb)); break;
    default: limbs_out = false; break;
  }
  if (limbs_out) {
    const auto& pr = R::plain(r);
    for (int i = 0; i < 9; ++i) out[i] = pr.l[i];
  }
}

// Fp2 over raw limbs: an operand is 18 limbs (c0 | c1), both components of one class.  op: 0 mul, 1 sqr, 2 mul2sub, 3 inv
template <class G>
KG_HD void raw2_case(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, const double* bnd, uint32_t* out) {
  using R = Raw<G>;
  using F2 = Fp2<G>;
  const double* ba = bnd; const double* bb = bnd ? bnd + 3 : nullptr; const double* bc = bnd ? bnd + 6 : nullptr; const double* bd = bnd ? bnd + 9 : nullptr;
  for (int i = 0; i < RAW_OUT; ++i) out[i] = 0;
  F2 r = F2::zero();
  switch (op) {
    case 0: r = mul(F2{R::limbs(a, ba), R::limbs(a + 9, ba)}, F2{R::limbs(b, bb), R::limbs(b + 9, bb)}); break;
    case 1: r = sqr(F2{R::limbs(a, ba), R::limbs(a + 9, ba)}); break;
    case 2: r = mul2sub(F2{R::limbs(a, ba), R::limbs(a + 9, ba)}, F2{R::limbs(b, bb), R::limbs(b + 9, bb)},
                        F2{R::limbs(c, bc), R::limbs(c + 9, bc)}, F2{R::limbs(d, bd), R::limbs(d + 9, bd)}); break;
    case 3: r = inv(F2{R::limbs(a, ba), R::limbs(a + 9, ba)}); break;
    default: break;
  }
  const auto& p0 = R::plain(r.c0);
  const auto& p1 = R::plain(r.c1);
  for (int i = 0; i < 9; ++i) { out[i] = p0.l[i]; out[9 + i] = p1.l[i]; }
}

// ---- one-lane point formulas (curve.h) ------------------------------------------------------------------------------------------------------
// a point in memory read and written coordinate by coordinate: the device's SoaSrc / SoaDst / AosSrc accessors over one slot
template <class F> struct MemPt {
  XYZZ<F>* s;
  KG_HD F x() const { return s->x; }
  KG_HD F y() const { return s->y; }
  KG_HD F zz() const { return s->zz; }
  KG_HD F zzz() const { return s->zzz; }
  KG_HD void x(const F& v) const { s->x = v; }
  KG_HD void y(const F& v) const { s->y = v; }
  KG_HD void zz(const F& v) const { s->zz = v; }
  KG_HD void zzz(const F& v) const { s->zzz = v; }
};
enum CurveOp { C_DOUBLE_AFFINE = 0, C_DOUBLE_XYZZ, C_ADD_MIXED, C_ADD_MIXED_POS, C_ADD_MIXED_NEG, C_ADD_XYZZ, C_ADD_XYZZ_STREAM, C_DOUBLE_XYZZ_STREAM,
               C_NEG_XYZZ, C_TO_AFFINE };
// p, q: X, Y, ZZ, ZZZ in the ABI form (4 x Conv<F>::W words; all zero: the identity); the affine operand of a formula is (X, Y) of q, the
// doubled affine point of C_DOUBLE_AFFINE too.  The result goes through to_affine: o = x | y in the ABI form, returns 1 for the identity.
// (C_DOUBLE_XYZZ_STREAM: p is not the identity -- its callers filter it.)
template <class F>
KG_HD XYZZ<F> xyzz_in(const uint32_t* p) {
  constexpr int W = Conv<F>::W;
  return {Conv<F>::in(p), Conv<F>::in(p + W), Conv<F>::in(p + 2 * W), Conv<F>::in(p + 3 * W)};
}
template <class F>
KG_HD int affine_out(const XYZZ<F>& r, uint32_t* o) {
  constexpr int W = Conv<F>::W;
  Affine<F> af;
  if (!to_affine(r, af)) {
    for (int i = 0; i < 2 * W; ++i) o[i] = 0;
    return 1;
  }
  Conv<F>::out(af.x, o);
  Conv<F>::out(af.y, o + W);
  return 0;
}
template <class F>
KG_HD int curve_case(int op, const uint32_t* p, const uint32_t* q, uint32_t* o) {
  const XYZZ<F> P = xyzz_in<F>(p);
  XYZZ<F> Q = xyzz_in<F>(q);
  const Affine<F> qa{Q.x, Q.y};
  XYZZ<F> r = P;
  switch (op) {
    case C_DOUBLE_AFFINE: r = double_affine(qa); break;
    case C_DOUBLE_XYZZ: r = double_xyzz(P); break;
    case C_ADD_MIXED: r = add_mixed(P, qa); break;
    case C_ADD_MIXED_POS: r = add_mixed_signed(P, qa, false); break;
    case C_ADD_MIXED_NEG: r = add_mixed_signed(P, qa, true); break;
    case C_ADD_XYZZ: r = add_xyzz(P, Q); break;
    case C_ADD_XYZZ_STREAM: { MemPt<F> s{&r}, t{&Q}, u{&r}; add_xyzz_stream<F>(s, t, u); break; }       // in place on the first operand
    case C_DOUBLE_XYZZ_STREAM: { MemPt<F> s{&r}, u{&r}; double_xyzz_stream<F>(s, u); break; }
    case C_NEG_XYZZ: r = neg_xyzz(P); break;
    default: break;
  }
  return affine_out<F>(r, o);
}

// ---- lane-cooperative formulas (coop_add.h) -------------------------------------------------------------------------------------------------
// One wave works on an image of COOP_ITEMS points; quad t of its 16 quads gets (ia, ib, io, active, doublings): io <- ia + ib when active, then
// io doubled `doublings` (<= COOP_MAX_DBL) times.  The quads of a wave work on disjoint items (the caller's rule: the device runs them at once).
constexpr uint32_t COOP_ITEMS = 48, COOP_QUADS = 16, COOP_PARAMS = 5, COOP_MAX_DBL = 3;
KG_HD bool coop_params_ok(const uint32_t* pr) { return pr[0] < COOP_ITEMS && pr[1] < COOP_ITEMS && pr[2] < COOP_ITEMS && pr[4] <= COOP_MAX_DBL; }

// ---- digits (msm_digits.h) ------------------------------------------------------------------------------------------------------------------
// signed window digits of a canonical integer k: digits[w], w < W = ceil(255 / c) <= 128; returns W
KG_HD int small_digits_case(const uint32_t* k, int c, int32_t* digits) {
  const int W = (255 + c - 1) / c;
  uint32_t H[8];
  small_bias(c, W, H);
  uint32_t kb[8];
  uint64_t cy = 0;
  for (int j = 0; j < 8; ++j) { const uint64_t s_ = (uint64_t)k[j] + H[j] + cy; kb[j] = (uint32_t)s_; cy = s_ >> 32; }
  for (int w = 0; w < W; ++w) {
    bool neg;
    const uint32_t m = small_window_digit(kb, w, c, W, neg);
    digits[w] = neg ? -(int32_t)m : (int32_t)m;
  }
  return W;
}
// GLV decomposition: k (canonical, 8 words) -> |k1|, |k2| (4 words each) and their signs
template <class L>
KG_HD void glv_decompose_case(const uint32_t* k, uint32_t* k1, uint32_t* k2, uint8_t* neg) {
  bool n1, n2;
  uint32_t a[4], b[4];
  glv_decompose_with<L>(k, a, n1, b, n2);
  for (int j = 0; j < 4; ++j) { k1[j] = a[j]; k2[j] = b[j]; }
  neg[0] = n1; neg[1] = n2;
}
// The whole digit path of a scalar with halved scalars (glv): decomposition, |k_e| + H over W = ceil(128 / c) windows, signed digits with the
// half's sign folded in.  digits: [2][64] (window w of half e); returns W.
template <class L>
KG_HD int glv_digits_case(const uint32_t* k, int c, int32_t* digits) {
  const int W = (128 + c - 1) / c;
  uint32_t H[8];
  small_bias(c, W, H);
  uint32_t ks[2][8];
  bool ng[2];
  glv_decompose_with<L>(k, ks[0], ng[0], ks[1], ng[1]);
  for (int e = 0; e < 2; ++e) {
    uint64_t cy = 0;
    for (int j = 0; j < 4; ++j) { const uint64_t s_ = (uint64_t)ks[e][j] + H[j] + cy; ks[e][j] = (uint32_t)s_; cy = s_ >> 32; }
    for (int j = 4; j < 8; ++j) ks[e][j] = 0;
    for (int w = 0; w < W; ++w) {
      bool neg;
      const uint32_t m = small_window_digit(ks[e], w, c, W, neg);
      digits[e * 64 + w] = (neg != ng[e]) ? -(int32_t)m : (int32_t)m;
    }
  }
  return W;
}

}  // namespace kgcase
