// acc_abi_bases_host.cpp -- the accumulation's third base format (BASES_ABI: the caller's array gathered as it is, msm_bases.h
// load_point_abi) on the host, as a stand-alone program: the unpack with the factor 32 in its shifts (fp29.h limbs_from_words_x32), the
// conversion the exceptional branches do first (from_ref_x32) and add_mixed_signed(..., abi = true) (curve.h), once on the plain types
// and once on the bound-tracking FpChecked types, which abort when a 64-bit column, a 32-bit limb or a Montgomery value bound of fp29.h
// could be exceeded.
//
//   acc_abi_bases_host <points file>
//
// points file: per curve a record  u32 field (0 = Fq: G1, 1 = Fr: Grumpkin), u32 n, n x 8 u64 (x | y in the ABI's reference form).
// Prints one line "ok ..." and exits 0; any mismatch prints what failed and exits 1; a bound violation aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/fp29_checked.h"
#include "../../kogarashi_amd/csrc/curve.h"

using namespace kg;

static long g_checks = 0;
[[noreturn]] static void die(const char* what, long at) {
  std::fprintf(stderr, "acc_abi_bases_host: %s (case %ld)\n", what, at);
  std::exit(1);
}

// how a field type enters: the two forms of a base coordinate, and an accumulator carrying the bounds the kernel's comments document
template <class F> struct In;
template <class P> struct In<Fp<P>> {
  using Prm = P;
  static Fp<P> abi(const uint32_t* w) { return limbs_from_words_x32<P>(w); }
  static Fp<P> resident(const uint32_t* w) { return from_ref<P>(w); }
  static XYZZ<Fp<P>> at_maxima(const XYZZ<Fp<P>>& p) { return p; }
  static const Fp<P>& raw(const Fp<P>& a) { return a; }
};
template <class P> struct In<FpChecked<P>> {
  using Prm = P;
  static FpChecked<P> abi(const uint32_t* w) { return checked_from_words_x32<P>(w); }      // K = 32, top limb < 32 (PTOP + 1)
  static FpChecked<P> resident(const uint32_t* w) {                                         // from_ref on a canonical value
    return mul(FpChecked<P>::wrap(limbs_from_words<P>(w), 1.0), FpChecked<P>::from_const(P::C_FROM_REF));
  }
  // curve.h add_mixed_signed: X < 6p (kept without a value reduction), Y, ZZ, ZZZ < 2p (products); whatever the values are
  static XYZZ<FpChecked<P>> at_maxima(const XYZZ<FpChecked<P>>& p) {
    if (is_zero_2p(p.zz.v)) return p;
    return {FpChecked<P>::wrap(p.x.v, 6.0), FpChecked<P>::wrap(p.y.v, 2.0), FpChecked<P>::wrap(p.zz.v, 2.0), FpChecked<P>::wrap(p.zzz.v, 2.0)};
  }
  static const Fp<P>& raw(const FpChecked<P>& a) { return a.v; }
};

template <class F> static Affine<F> abi_point(const uint32_t* w) { return {In<F>::abi(w), In<F>::abi(w + 8)}; }
template <class F> static Affine<F> resident_point(const uint32_t* w) { return {In<F>::resident(w), In<F>::resident(w + 8)}; }

template <class F> static bool same_limbs_xyzz(const XYZZ<F>& a, const XYZZ<F>& b) {
  return same_limbs(In<F>::raw(a.x), In<F>::raw(b.x)) && same_limbs(In<F>::raw(a.y), In<F>::raw(b.y)) &&
         same_limbs(In<F>::raw(a.zz), In<F>::raw(b.zz)) && same_limbs(In<F>::raw(a.zzz), In<F>::raw(b.zzz));
}
// the same group element (accumulators hold different representatives of a coordinate: compare the canonical affine point)
template <class F> static bool same_point(const XYZZ<F>& a, const XYZZ<F>& b) {
  Affine<F> pa, pb;
  const bool ia = !to_affine(a, pa), ib = !to_affine(b, pb);
  if (ia || ib) return ia == ib;
  return same_limbs(In<F>::raw(reduce(pa.x)), In<F>::raw(reduce(pb.x))) && same_limbs(In<F>::raw(reduce(pa.y)), In<F>::raw(reduce(pb.y)));
}

struct Rng {
  uint64_t s;
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
};

// the words of 0, 1, p - 1 as raw reference values, of the field's 0, 1, p - 1 (x * 2^256 mod p), and random canonical values
template <class P> static std::vector<std::vector<uint32_t>> coordinate_values(int nrandom) {
  std::vector<std::vector<uint32_t>> v;
  uint32_t pm1[8], one[8] = {1, 0, 0, 0, 0, 0, 0, 0}, zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8];
  Fp<P> m = Fp<P>::from_const(P::P);
  m.l[0] -= 1;
  words_from_limbs(m, pm1);
  for (const uint32_t* k : {zero, one, pm1}) {
    v.emplace_back(k, k + 8);
    int_to_ref<P>(k, w);
    v.emplace_back(w, w + 8);
  }
  Rng r{0x9E3779B97F4A7C15ull};
  for (int i = 0; i < nrandom; ++i) {
    for (int j = 0; j < 8; j += 2) { const uint64_t x = r.next(); w[j] = (uint32_t)x; w[j + 1] = (uint32_t)(x >> 32); }
    w[7] &= (i & 1) ? 0x1fffffffu : 0x2fffffffu;      // < 2^253 or < 0x30000000 * 2^224: both below p = 0x30644e72...
    v.emplace_back(w, w + 8);
  }
  return v;
}

// 1. load_point_abi's unpack followed by the exceptional branches' conversion is from_ref, limb for limb
template <class F> static void conversion_is_from_ref() {
  using P = typename In<F>::Prm;
  long at = 0;
  for (const auto& w : coordinate_values<P>(4000)) {
    const F a = In<F>::abi(w.data());
    const Fp<P>& al = In<F>::raw(a);
    for (int j = 0; j < 9; ++j)
      if (al.l[j] > M29) die("unpacked limb not normalised", at);
    const Fp<P> ref = limbs_from_words<P>(w.data());
    if (!same_limbs(limbs_div32(al), ref)) die("limbs_from_words_x32 is not 32 x limbs_from_words", at);
    if (!same_limbs(In<F>::raw(from_ref_x32(a)), from_ref<P>(w.data()))) die("from_ref_x32(unpack) differs from from_ref", at);
    ++at; ++g_checks;
  }
}

// 2. bounds at the extremes: every pair of coordinate values 0, 1, p - 1 (raw and as field elements) as a base -- the formulas' bounds do not
// depend on the point lying on the curve -- against an accumulator at its documented maxima, both signs; and through the three exits that
// take the base as a value: a first entry, a doubling (the accumulator IS the base), the negation of either.  The ABI route must give what
// the resident route gives.
template <class F> static void extremes(const XYZZ<F>& some_acc) {
  using P = typename In<F>::Prm;
  const auto vals = coordinate_values<P>(2);
  long at = 0;
  for (const auto& x : vals)
    for (const auto& y : vals) {
      uint32_t w[16];
      std::memcpy(w, x.data(), 32); std::memcpy(w + 8, y.data(), 32);
      const Affine<F> a = abi_point<F>(w), b = resident_point<F>(w);
      for (int neg = 0; neg < 2; ++neg) {
        const XYZZ<F> acc = In<F>::at_maxima(some_acc);
        (void)add_mixed_signed(acc, a, neg != 0, true);                       // the main addition (or, by chance, an exit): bounds only
        const XYZZ<F> first = add_mixed_signed(XYZZ<F>::identity(), a, neg != 0, true);
        if (!same_limbs_xyzz(first, add_mixed_signed(XYZZ<F>::identity(), b, neg != 0, false))) die("first entry differs", at);
        // the accumulator is the base itself: equal x; same sign -> doubling, opposite sign -> identity (y = 0: both at once, bounds only)
        for (int neg2 = 0; neg2 < 2; ++neg2) {
          const XYZZ<F> r1 = add_mixed_signed(In<F>::at_maxima(first), a, neg2 != 0, true);
          const XYZZ<F> r2 = add_mixed_signed(In<F>::at_maxima(first), b, neg2 != 0, false);
          if (!same_limbs_xyzz(r1, r2)) die("equal-x exit differs", at);
          g_checks += 1;
        }
        ++at;
      }
    }
}

// 3. real points: a fold over the file's points by both routes (first entry, main additions with either sign), then every exceptional branch
// from an accumulator with ZZ != 1: P + P (doubling), P - P (identity), and a first entry again
template <class F> static XYZZ<F> points(const std::vector<uint64_t>& pts) {
  const size_t n = pts.size() / 8;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(pts.data());
  XYZZ<F> acc_abi = XYZZ<F>::identity(), acc_res = XYZZ<F>::identity();
  for (size_t i = 0; i < n; ++i) {
    const bool neg = (i % 3) == 1;
    acc_abi = add_mixed_signed(In<F>::at_maxima(acc_abi), abi_point<F>(w + 16 * i), neg, true);
    acc_res = add_mixed_signed(acc_res, resident_point<F>(w + 16 * i), neg, false);
    if (!same_point(acc_abi, acc_res)) die("fold differs", (long)i);
    ++g_checks;
  }
  for (size_t i = 0; i + 1 < n; ++i) {
    const uint32_t* wp = w + 16 * i;
    const uint32_t* wq = w + 16 * (i + 1);
    if (!std::memcmp(wp, wq, 32)) continue;                                  // equal x: the pair below would not come back to P
    // P as an accumulator with a non-trivial ZZ: (P + Q) - Q
    XYZZ<F> p = add_mixed_signed(XYZZ<F>::identity(), abi_point<F>(wp), false, true);
    p = add_mixed_signed(p, abi_point<F>(wq), false, true);
    p = add_mixed_signed(p, abi_point<F>(wq), true, true);
    const Affine<F> b = resident_point<F>(wp);
    const XYZZ<F> twice = add_mixed_signed(In<F>::at_maxima(p), abi_point<F>(wp), false, true);
    if (!same_limbs_xyzz(twice, double_affine(b))) die("doubling exit not taken or differs", (long)i);
    const XYZZ<F> ntwice = add_mixed_signed(neg_xyzz(p), abi_point<F>(wp), true, true);
    if (!same_limbs_xyzz(ntwice, double_affine(neg_affine(b)))) die("negated doubling exit not taken or differs", (long)i);
    const XYZZ<F> none = add_mixed_signed(In<F>::at_maxima(p), abi_point<F>(wp), true, true);
    if (!is_identity(none)) die("P - P is not the identity", (long)i);
    const XYZZ<F> again = add_mixed_signed(none, abi_point<F>(wq), true, true);
    if (!same_limbs_xyzz(again, from_affine(neg_affine(resident_point<F>(wq))))) die("first entry after the identity differs", (long)i);
    g_checks += 4;
  }
  return acc_abi;
}

template <class P> static void run_field(const std::vector<uint64_t>& pts) {
  conversion_is_from_ref<Fp<P>>();
  conversion_is_from_ref<FpChecked<P>>();
  const XYZZ<Fp<P>> a = points<Fp<P>>(pts);
  const XYZZ<FpChecked<P>> c = points<FpChecked<P>>(pts);
  if (!same_limbs_xyzz(a, XYZZ<Fp<P>>{c.x.v, c.y.v, c.zz.v, c.zzz.v})) die("checked and plain folds differ", 0);
  extremes<Fp<P>>(a);
  extremes<FpChecked<P>>(c);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <points file>\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int records = 0;
  for (;;) {
    uint32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2) break;
    if (hdr[0] > 1 || hdr[1] < 2 || hdr[1] > 100000) die("bad record header", records);
    std::vector<uint64_t> pts((size_t)hdr[1] * 8);
    if (std::fread(pts.data(), 8, pts.size(), f) != pts.size()) die("short record", records);
    if (hdr[0] == 0) run_field<FqParams>(pts); else run_field<FrParams>(pts);
    ++records;
  }
  std::fclose(f);
  if (records == 0) die("no records", 0);
  std::printf("ok records=%d checks=%ld\n", records, g_checks);
  return 0;
}
