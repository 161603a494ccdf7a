// nova_fold_batch_host.cpp -- the parts of a batched Nova fold (kg_nova_cross_term_batch, kg_field_vec_axpy_batch: kogarashi_amd/csrc/vec.hip;
// kg_points_muladd_batch: kogarashi_amd/csrc/points_fold.hip) that need no device, as a stand-alone program: tests/test_nova_fold_batch_host.py
// builds it with g++, plain -- which includes the bound-tracking type -- and with -fsanitize=address,undefined, and runs it.
//
//   nova_fold_batch_host             every section; prints one "ok: ..." line per section, exits non-zero at the first failing section
//
//   args    nova_cross_batch_args_ok (r1cs_batch.h), axpy_batch_args_ok, points_muladd_args_ok (nova_batch.h), the headers alone: every
//           refusal and every accepted empty call of the three entries
//   cross   cross_term_row (vecops.h) fed with u_factor-scaled u1 and u2 -- the batch's device path -- against the same row fed with
//           u_scaled_words' canonical values -- the single call's host path -- and against the row's value in the host's field type, for
//           (u1, u2) in {0, 1, p - 1, random}^2 over both fields, on the device type and on the bound-checked type; then with row sums
//           at their documented maximum (raw words of 2^256 - 1 accumulated, tracked below 1.06p)
//   axpy    axpy_step (vecops.h: the batch kernel's body) with non-canonical raw words as a and b and s in {0, 1, p - 1, random}
//           against the host's field type
//   index   axpy_batch_at and points_muladd_scalar_at: the lane -> (vector, element) rule and the per_scalar rule
//   chain   P + k Q by muladd_chain_ops (groth16_assemble.h: what k_points_muladd runs, from the scalar's Montgomery words) over the
//           device's field type, the bound-tracking type (255 chained steps machine-checked) and the host's type, on G1 and on Grumpkin,
//           against a plain double-and-add: k in {0, 1, 2, p - 1, 2^127, random}; P, Q or both the identity; P = Q; P = -Q with k = 1;
//           P = -k Q (the identity)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/r1cs_batch.h"
#include "../../kogarashi_amd/csrc/nova_batch.h"
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/vecops.h"
#include "../../kogarashi_amd/csrc/host_fp.h"
#include "../../kogarashi_amd/csrc/groth16_assemble.h"
#ifndef KG_NOVA_HOST_PLAIN_ONLY
#include "../../kogarashi_amd/csrc/fp29_checked.h"
#endif

using namespace kg;

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct Csr { const void *d_row_ptr, *d_col, *d_val; };

// ---- args ---------------------------------------------------------------------------------------------------------------------------
static void test_args() {
  int some;                                               // any non-null address: nothing is dereferenced
  const void* p = &some;
  const Csr full{p, p, p}, no_rows{nullptr, p, p}, no_col{p, nullptr, p}, no_val{p, p, nullptr};
  const size_t big = (size_t)1 << 32, over = SIZE_MAX / 32 / 3 + 1;
  auto cok = [&](const void* ctx, int field, const Csr* a, const Csr* b, const Csr* c, size_t m, const void* z1, size_t s1, const void* z2, size_t s2, size_t count,
                 const void* out, size_t so) { return nova_cross_batch_args_ok(ctx, field, a, b, c, m, z1, s1, z2, s2, count, out, so); };
  EXPECT(cok(p, 0, &full, &full, &full, 5, p, 9, p, 9, 3, p, 5));
  EXPECT(cok(p, 1, &full, &full, &full, 5, p, 11, p, 9, 3, p, 8));                   // wider strides, differing between z1 and z2
  EXPECT(cok(p, 0, &full, &full, &full, 5, p, 0, p, 0, 3, p, 5));                    // the z strides are trusted (0: one vector count times)
  EXPECT(cok(p, 0, &full, &full, &full, big - 1, p, 9, p, 9, 3, p, big - 1));
  EXPECT(!cok(nullptr, 0, &full, &full, &full, 5, p, 9, p, 9, 3, p, 5));             // a null ctx
  EXPECT(!cok(nullptr, 0, &full, &full, &full, 0, p, 9, p, 9, 0, p, 5));             //   even for an empty call
  EXPECT(!cok(p, 2, &full, &full, &full, 5, p, 9, p, 9, 3, p, 5));                   // an unknown field
  EXPECT(!cok(p, -1, &full, &full, &full, 5, p, 9, p, 9, 0, p, 5));                  //   even for an empty call
  EXPECT(!cok(p, 0, &full, &full, &full, big, p, 9, p, 9, 3, p, big));               // m >= 2^32
  EXPECT(!cok(p, 0, &full, &full, &full, big, p, 9, p, 9, 0, p, big));               //   even for an empty call
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, 9, p, 9, 3, p, 4));                   // out_stride < m
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, 9, p, 9, 0, p, 4));                   //   even for an empty call
  EXPECT(!cok(p, 0, nullptr, &full, &full, 5, p, 9, p, 9, 3, p, 5));                 // a null kg_csr, each position
  EXPECT(!cok(p, 0, &full, nullptr, &full, 5, p, 9, p, 9, 3, p, 5));
  EXPECT(!cok(p, 0, &full, &full, nullptr, 5, p, 9, p, 9, 3, p, 5));
  EXPECT(!cok(p, 0, &no_rows, &full, &full, 5, p, 9, p, 9, 3, p, 5));                // a null member array, each member
  EXPECT(!cok(p, 0, &full, &no_col, &full, 5, p, 9, p, 9, 3, p, 5));
  EXPECT(!cok(p, 0, &full, &full, &no_val, 5, p, 9, p, 9, 3, p, 5));
  EXPECT(!cok(p, 0, &full, &full, &full, 5, nullptr, 9, p, 9, 3, p, 5));             // a null d_z1, d_z2, d_out
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, 9, nullptr, 9, 3, p, 5));
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, 9, p, 9, 3, nullptr, 5));
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, over, p, 9, 3, p, 5));                // count * stride * 32 beyond size_t: z1, z2, out
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, 9, p, over, 3, p, 5));
  EXPECT(!cok(p, 0, &full, &full, &full, 5, p, 9, p, 9, 3, p, over));
  EXPECT(cok(p, 0, &full, &full, &full, 5, p, over - 1, p, over - 1, 3, p, over - 1));
  EXPECT(cok(p, 0, nullptr, nullptr, nullptr, 5, nullptr, 0, nullptr, 0, 0, nullptr, 5));       // count == 0: nothing is looked at
  EXPECT(cok(p, 1, &no_val, nullptr, &full, 0, nullptr, 0, nullptr, 0, 3, nullptr, 0));         // m == 0

  auto aok = [&](const void* ctx, int field, const void* a, size_t sa, const void* s, const void* b, size_t sb, const void* out, size_t so, size_t n, size_t count) {
    return axpy_batch_args_ok(ctx, field, a, sa, s, b, sb, out, so, n, count);
  };
  EXPECT(aok(p, 0, p, 7, p, p, 7, p, 7, 7, 3) && aok(p, 1, p, 9, p, p, 8, p, 7, 7, 3));
  EXPECT(!aok(nullptr, 0, p, 7, p, p, 7, p, 7, 7, 3) && !aok(nullptr, 0, p, 7, p, p, 7, p, 7, 0, 0));          // a null ctx, even when empty
  EXPECT(!aok(p, 2, p, 7, p, p, 7, p, 7, 7, 3) && !aok(p, -1, p, 7, p, p, 7, p, 7, 7, 0));                     // an unknown field, even when empty
  EXPECT(!aok(p, 0, p, 6, p, p, 7, p, 7, 7, 3) && !aok(p, 0, p, 7, p, p, 6, p, 7, 7, 3) && !aok(p, 0, p, 7, p, p, 7, p, 6, 7, 3));      // a stride below n
  EXPECT(!aok(p, 0, p, 6, p, p, 7, p, 7, 7, 0));                                                               //   even when empty
  EXPECT(!aok(p, 0, nullptr, 7, p, p, 7, p, 7, 7, 3) && !aok(p, 0, p, 7, nullptr, p, 7, p, 7, 7, 3) && !aok(p, 0, p, 7, p, nullptr, 7, p, 7, 7, 3) &&
         !aok(p, 0, p, 7, p, p, 7, nullptr, 7, 7, 3));                                                         // a null array, each
  EXPECT(!aok(p, 0, p, over, p, p, 7, p, 7, 7, 3) && !aok(p, 0, p, 7, p, p, over, p, 7, 7, 3) && !aok(p, 0, p, 7, p, p, 7, p, over, 7, 3));
  EXPECT(aok(p, 0, p, over - 1, p, p, 7, p, 7, 7, 3));
  EXPECT(aok(p, 0, nullptr, 7, nullptr, nullptr, 7, nullptr, 7, 7, 0) && aok(p, 1, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 0, 3));         // the empty calls

  auto pok = [&](const void* ctx, int curve, const void* pp, const void* q, const void* k, size_t per, size_t count, const void* out, const void* oinf) {
    return points_muladd_args_ok(ctx, curve, pp, q, k, per, count, out, oinf);
  };
  EXPECT(pok(p, 0, p, p, p, 1, 5, p, p) && pok(p, 1, p, p, p, 2, 6, p, p) && pok(p, 0, p, p, p, 7, 5, p, p));
  EXPECT(!pok(nullptr, 0, p, p, p, 1, 5, p, p) && !pok(nullptr, 0, p, p, p, 1, 0, p, p));                      // a null ctx, even when empty
  EXPECT(!pok(p, 2, p, p, p, 1, 5, p, p) && !pok(p, 2, p, p, p, 1, 0, p, p) && !pok(p, -1, p, p, p, 1, 5, p, p) && !pok(p, 3, p, p, p, 1, 5, p, p));   // G2, unknown
  EXPECT(!pok(p, 0, p, p, p, 0, 5, p, p) && !pok(p, 0, p, p, p, 0, 0, p, p));                                  // per_scalar == 0, even when empty
  EXPECT(!pok(p, 0, nullptr, p, p, 1, 5, p, p) && !pok(p, 0, p, nullptr, p, 1, 5, p, p) && !pok(p, 0, p, p, nullptr, 1, 5, p, p) &&
         !pok(p, 0, p, p, p, 1, 5, nullptr, p) && !pok(p, 0, p, p, p, 1, 5, p, nullptr));                      // a null array, each
  EXPECT(!pok(p, 0, p, p, p, 1, (size_t)1 << 37, p, p) && pok(p, 0, p, p, p, 1, ((size_t)1 << 37) - 1, p, p));
  EXPECT(pok(p, 1, nullptr, nullptr, nullptr, 2, 0, nullptr, nullptr));                                        // count == 0
  if (!failures) std::printf("ok: args\n");
}

// ---- the field sections' plumbing -----------------------------------------------------------------------------------------------------
template <class F> struct RawIn;
template <class P> struct RawIn<Fp<P>> {
  static Fp<P> in(const uint32_t* w) { return limbs_from_words<P>(w); }
  static Fp<P> internal(const uint32_t* w) { return from_ref<P>(w); }
  static const Fp<P>& plain(const Fp<P>& x) { return x; }
};
#ifndef KG_NOVA_HOST_PLAIN_ONLY
template <class P> struct RawIn<FpChecked<P>> {
  static FpChecked<P> in(const uint32_t* w) { return FpChecked<P>::wrap(limbs_from_words<P>(w), 5.4); }      // any 256-bit input
  static FpChecked<P> internal(const uint32_t* w) { return mul(in(w), FpChecked<P>::from_const(P::C_FROM_REF)); }
  static const Fp<P>& plain(const FpChecked<P>& x) { return x.v; }
};
#endif
template <class H> static std::vector<H> field_values() {      // 0, 1, p - 1 and values off a fixed chain, with their negatives
  const H one = H::one(), zero = H::zero();
  std::vector<H> v = {zero, one, sub<4, 1>(zero, one)};
  H rnd = one;
  for (int i = 0; i < 6; ++i) {
    for (int k = 0; k < 3; ++k) rnd = add(dbl(rnd), add(rnd, one));
    rnd = sqr(rnd);
    v.push_back(rnd);
    v.push_back(sub<4, 1>(zero, rnd));
  }
  return v;
}
template <class F> static void words_of(const F& canonical_2p, uint32_t out[8]) { words_from_limbs(RawIn<F>::plain(reduce_2p(canonical_2p)), out); }

// ---- cross ----------------------------------------------------------------------------------------------------------------------------
template <class F, class HostP>
static void cross_cases(const char* what) {
  using P = typename F::Params;
  using H = HostFp<HostP>;
  const std::vector<H> vals = field_values<H>();
  const H us[4] = {vals[0], vals[1], vals[2], vals[5]};
  // six row sums of one term each, z * v with both factors canonical Montgomery values: the row's value is known in the host's type
  H zv[6][2];
  F sum[6];
  for (int q = 0; q < 6; ++q) {
    zv[q][0] = vals[3 + q];
    zv[q][1] = vals[9 + (q % 5)];
    uint32_t wz[8], wv[8];
    std::memcpy(wz, zv[q][0].v, 32);
    std::memcpy(wv, zv[q][1].v, 32);
    sum[q] = dot_step(F::zero(), RawIn<F>::in(wz), RawIn<F>::in(wv));
  }
  // ... and six at the documented maximum: 40 terms of (2^256 - 1)^2 each, whatever their residue is
  F fat[6];
  {
    uint32_t ones[8];
    std::memset(ones, 0xff, sizeof ones);
    for (int q = 0; q < 6; ++q) {
      fat[q] = F::zero();
      for (int t = 0; t < 40 + q; ++t) fat[q] = dot_step(fat[q], RawIn<F>::in(ones), RawIn<F>::in(ones));
      fat[q] = dot_merge(fat[q], fat[q]);
    }
  }
  for (const H& u1 : us)
    for (const H& u2 : us) {
      uint64_t s1[4], s2[4];
      u_scaled_words<HostP>(u1.v, s1);                    // the single call's host path: ten doublings, canonical
      u_scaled_words<HostP>(u2.v, s2);
      uint32_t w1[8], w2[8], r1[8], r2[8];
      std::memcpy(w1, s1, 32); std::memcpy(w2, s2, 32);
      std::memcpy(r1, u1.v, 32); std::memcpy(r2, u2.v, 32);
      const Fp<P> l1 = limbs_from_words<P>(w1), l2 = limbs_from_words<P>(w2);
      const F h1 = F::from_const(l1.l), h2 = F::from_const(l2.l);
      const F d1 = u_factor(RawIn<F>::in(r1), F::from_const(P::C_XT_U)), d2 = u_factor(RawIn<F>::in(r2), F::from_const(P::C_XT_U));      // the batch's device path
      const F had = F::from_const(P::C_XT_HAD);
      uint32_t got_dev[8], got_host[8], want[8];
      words_of(cross_term_row(sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], d1, d2, had), got_dev);
      words_of(cross_term_row(sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], h1, h2, had), got_host);
      // az1 bz2 + az2 bz1 - u1 cz2 - u2 cz1 with (az1, az2, bz1, bz2, cz1, cz2) = sums 0 .. 5
      auto val = [&](int q) { return mul(zv[q][0], zv[q][1]); };
      const H t = sub<4, 1>(sub<4, 1>(add(mul(val(0), val(3)), mul(val(1), val(2))), mul(u1, val(5))), mul(u2, val(4)));
      std::memcpy(want, t.v, 32);
      if (std::memcmp(got_dev, got_host, 32) != 0 || std::memcmp(got_dev, want, 32) != 0) { std::fprintf(stderr, "%s: cross_term_row differs\n", what); ++failures; }
      words_of(cross_term_row(fat[0], fat[1], fat[2], fat[3], fat[4], fat[5], d1, d2, had), got_dev);
      words_of(cross_term_row(fat[0], fat[1], fat[2], fat[3], fat[4], fat[5], h1, h2, had), got_host);
      if (std::memcmp(got_dev, got_host, 32) != 0) { std::fprintf(stderr, "%s: cross_term_row differs at the maximum\n", what); ++failures; }
    }
  if (!failures) std::printf("ok: cross %s\n", what);
}

// ---- axpy -----------------------------------------------------------------------------------------------------------------------------
template <class F, class HostP>
static void axpy_cases(const char* what) {
  using H = HostFp<HostP>;
  const std::vector<H> vals = field_values<H>();
  const H ss[4] = {vals[0], vals[1], vals[2], vals[7]};
  uint32_t raws[5][8];
  std::memset(raws[0], 0xff, 32);                                                     // 2^256 - 1
  std::memset(raws[1], 0, 32);
  for (int i = 0; i < 8; ++i) { raws[2][i] = 0x80000000u >> i; raws[3][i] = 0xfffffff0u + i; }
  std::memcpy(raws[4], HostP::P, 32);                                                 // p itself: the value 0, not canonical
  for (const H& s : ss)
    for (auto& ra : raws)
      for (auto& rb : raws) {
        uint32_t ws[8], got[8];
        std::memcpy(ws, s.v, 32);
        words_of(axpy_step(RawIn<F>::in(ra), RawIn<F>::in(rb), RawIn<F>::internal(ws)), got);
        uint64_t a64[4], b64[4];
        std::memcpy(a64, ra, 32); std::memcpy(b64, rb, 32);
        const H a = mul(H::from_words(a64), H::one()), b = mul(H::from_words(b64), H::one());     // the raw words' residues (x R / R)
        const H t = add(a, mul(s, b));
        if (std::memcmp(got, t.v, 32) != 0) { std::fprintf(stderr, "%s: axpy_step differs\n", what); ++failures; }
      }
  if (!failures) std::printf("ok: axpy %s\n", what);
}

// ---- index ----------------------------------------------------------------------------------------------------------------------------
static void test_index() {
  for (size_t n : {(size_t)1, (size_t)2, (size_t)255, (size_t)257})
    for (size_t count : {(size_t)1, (size_t)5, (size_t)65537}) {
      if (n * count > 200000) continue;
      std::vector<int> seen(n * count, 0);
      for (size_t t = 0; t < n * count; ++t) {
        const AxpyBatchAt at = axpy_batch_at(t, n);
        EXPECT(at.vec < count && at.elem < n);
        ++seen[at.vec * n + at.elem];
      }
      for (int v : seen) EXPECT(v == 1);                    // every (vector, element) once
    }
  static_assert(axpy_batch_at(0, 1).vec == 0 && axpy_batch_at(5, 1).vec == 5 && axpy_batch_at(5, 1).elem == 0, "n = 1: a lane per vector");
  static_assert(axpy_batch_at(513, 257).vec == 1 && axpy_batch_at(513, 257).elem == 256, "the last element of vector 1");
  for (size_t per : {(size_t)1, (size_t)2, (size_t)3})
    for (size_t j = 0; j < 131; ++j) EXPECT(points_muladd_scalar_at(j, per) == j / per);
  static_assert(points_muladd_scalar_at(0, 2) == 0 && points_muladd_scalar_at(1, 2) == 0 && points_muladd_scalar_at(2, 2) == 1, "a fold's two points share r");
  static_assert(points_muladd_scalar_at(129, 3) == 43 && points_muladd_scalar_at(7, 1) == 7, "per_scalar 3 and 1");
  EXPECT(AXPY_BATCH_LAUNCH_MAX / 256 < ((size_t)1 << 31));                            // a launch's blocks fit the grid's x dimension
  if (!failures) std::printf("ok: index\n");
}

// ---- chain ----------------------------------------------------------------------------------------------------------------------------
// ABI words (4 x u64 per base-field element, Montgomery R = 2^256) <-> a field type
template <class F> struct Io;
template <class P> struct Io<Fp<P>> {
  static Fp<P> load(const uint64_t* w) { uint32_t v[8]; std::memcpy(v, w, 32); return from_ref<P>(v); }
  static void store(const Fp<P>& a, uint64_t* w) { uint32_t v[8]; to_ref(a, v); std::memcpy(w, v, 32); }
};
#ifndef KG_NOVA_HOST_PLAIN_ONLY
template <class P> struct Io<FpChecked<P>> {
  static FpChecked<P> load(const uint64_t* w) { uint32_t v[8]; std::memcpy(v, w, 32); return RawIn<FpChecked<P>>::internal(v); }
  static void store(const FpChecked<P>& a, uint64_t* w) {
    uint32_t v[8];
    words_from_limbs(reduce_2p(mul(a, FpChecked<P>::from_const(P::C_TO_REF))).v, v);
    std::memcpy(w, v, 32);
  }
};
#endif
template <class P> struct Io<HostFp<P>> {
  static HostFp<P> load(const uint64_t* w) { return HostFp<P>::from_words(w); }
  static void store(const HostFp<P>& a, uint64_t* w) { a.to_words(w); }
};
// a point travels between the types as the device hands it on: affine ABI words and a flag
struct PointWords { uint64_t xy[8]; bool inf; };
template <class F> PointWords to_words(const XYZZ<F>& p) {
  PointWords r;
  std::memset(r.xy, 0, sizeof r.xy);
  Affine<F> a;
  r.inf = !to_affine(p, a);
  if (!r.inf) { Io<F>::store(a.x, r.xy); Io<F>::store(a.y, r.xy + 4); }
  return r;
}
template <class F> XYZZ<F> from_words(const PointWords& w) {
  if (w.inf) return XYZZ<F>::identity();
  return from_affine(Affine<F>{Io<F>::load(w.xy), Io<F>::load(w.xy + 4)});
}
static bool same(const PointWords& a, const PointWords& b) { return a.inf == b.inf && (a.inf || std::memcmp(a.xy, b.xy, sizeof a.xy) == 0); }
// k * g by plain double-and-add over the canonical integer, most significant bit first
template <class F> XYZZ<F> scalar_mul(const XYZZ<F>& g, const uint32_t k[8]) {
  XYZZ<F> acc = XYZZ<F>::identity();
  for (int b = 255; b >= 0; --b) {
    acc = double_xyzz(acc);
    if ((k[b >> 5] >> (b & 31)) & 1) acc = add_xyzz(acc, g);
  }
  return acc;
}

// P + k Q over type T as k_points_muladd runs it: the scalar arrives in Montgomery words
template <class T, class SP> PointWords muladd_over(const PointWords& p, const PointWords& q, const uint32_t k_ref[8]) {
  const XYZZ<T> pp = from_words<T>(p), qq = from_words<T>(q);
  const G16ArrayOps<T> ops{{pp, qq, add_xyzz(pp, qq)}};
  return to_words(muladd_chain_ops<T, SP>(ops, k_ref));
}
template <class FP, class FC, class FH, class SP>
static void chain_case(const PointWords& p, const PointWords& q, const uint32_t k_int[8], const char* what, int want_identity = -1) {
  uint32_t k_ref[8];
  int_to_ref<SP>(k_int, k_ref);
  const PointWords want = to_words(add_xyzz(from_words<FP>(p), scalar_mul(from_words<FP>(q), k_int)));
  const PointWords got[3] = {muladd_over<FP, SP>(p, q, k_ref), muladd_over<FC, SP>(p, q, k_ref), muladd_over<FH, SP>(p, q, k_ref)};
  for (int t = 0; t < 3; ++t)
    if (!same(got[t], want) || (want_identity >= 0 && (int)want.inf != want_identity)) {
      ++failures;
      std::fprintf(stderr, "FAILED chain: type %d (%s)\n", t, what);
    }
}
// FP, FC, FH: the curve's base field as the device's, the bound-tracking and the host's type; SP: its scalar field; order: the group's
template <class FP, class FC, class FH, class SP>
static void chain_cases(const PointWords& gen, const uint64_t order[4], const char* what) {
  const uint32_t k5[8] = {5, 0, 0, 0, 0, 0, 0, 0}, k7[8] = {7, 0, 0, 0, 0, 0, 0, 0};
  const XYZZ<FP> G = from_words<FP>(gen);
  const PointWords P = to_words(scalar_mul(G, k5)), Q = to_words(scalar_mul(G, k7)), NQ = to_words(neg_xyzz(from_words<FP>(Q)));
  PointWords ID = P;
  ID.inf = true;
  uint32_t ks[6][8] = {{0}, {1}, {2}, {0}, {0, 0, 0, 0x80000000u}, {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 0x5cedc834u, 0x1082276bu, 0xf3a27251u, 0xf86c6a11u, 0x1d2c5e3fu}};
  std::memcpy(ks[3], order, 32);
  ks[3][0] -= 1;                                           // the order is odd: no borrow
  const char* names[6] = {"k = 0", "k = 1", "k = 2", "k = p - 1", "k = 2^127", "k random"};
  for (int i = 0; i < 6; ++i) {
    chain_case<FP, FC, FH, SP>(P, Q, ks[i], names[i]);
    chain_case<FP, FC, FH, SP>(ID, Q, ks[i], "P the identity");
    chain_case<FP, FC, FH, SP>(P, ID, ks[i], "Q the identity");
    chain_case<FP, FC, FH, SP>(ID, ID, ks[i], "both the identity", 1);
    chain_case<FP, FC, FH, SP>(Q, Q, ks[i], "P = Q");
    const PointWords NKQ = to_words(neg_xyzz(scalar_mul(from_words<FP>(Q), ks[i])));
    chain_case<FP, FC, FH, SP>(NKQ, Q, ks[i], "P = -k Q: the identity", 1);
  }
  chain_case<FP, FC, FH, SP>(NQ, Q, ks[1], "P = -Q with k = 1: the identity", 1);
  chain_case<FP, FC, FH, SP>(NQ, Q, ks[5], "P = -Q, k random");
  if (!failures) std::printf("ok: chain %s\n", what);
}
static PointWords g1_gen() {
  PointWords r;
  r.inf = false;
  const uint32_t k1[8] = {1, 0, 0, 0, 0, 0, 0, 0}, k2[8] = {2, 0, 0, 0, 0, 0, 0, 0};
  Io<Fq>::store(from_int<FqParams>(k1), r.xy);
  Io<Fq>::store(from_int<FqParams>(k2), r.xy + 4);
  return r;
}
static PointWords grumpkin_gen() {                         // (1, sqrt(-16)), y in Montgomery words (csrc/groth16.hip Gen<Fr>)
  PointWords r;
  r.inf = false;
  const uint32_t k1[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t y[8] = {0x448c41d8u, 0x11b2dff1u, 0x21c77dc3u, 0x23d3446fu, 0x35dfafbbu, 0xaa7b8cf4u, 0x9dc25d68u, 0x14b34cf6u};
  Io<Fr>::store(from_int<FrParams>(k1), r.xy);
  std::memcpy(r.xy + 4, y, 32);
  return r;
}

int main() {
  test_args();
  cross_cases<Fr, HostFrP>("Fr");
  cross_cases<Fq, HostFqP>("Fq");
  axpy_cases<Fr, HostFrP>("Fr");
  axpy_cases<Fq, HostFqP>("Fq");
#ifndef KG_NOVA_HOST_PLAIN_ONLY
  cross_cases<FrC, HostFrP>("Fr checked");
  cross_cases<FqC, HostFqP>("Fq checked");
  axpy_cases<FrC, HostFrP>("Fr checked");
  axpy_cases<FqC, HostFqP>("Fq checked");
#endif
  test_index();
#ifndef KG_NOVA_HOST_PLAIN_ONLY
  chain_cases<Fq, FqC, HostFq, FrParams>(g1_gen(), HostFrP::P, "G1");
  chain_cases<Fr, FrC, HostFr, FqParams>(grumpkin_gen(), HostFqP::P, "Grumpkin");
#else
  chain_cases<Fq, Fq, HostFq, FrParams>(g1_gen(), HostFrP::P, "G1");
  chain_cases<Fr, Fr, HostFr, FqParams>(grumpkin_gen(), HostFqP::P, "Grumpkin");
#endif
  if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
  std::printf("ok: nova fold batch host\n");
  return 0;
}
