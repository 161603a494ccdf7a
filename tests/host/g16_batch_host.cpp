// g16_batch_host.cpp -- the parts of the batched Groth16 prover (kg_groth16_prove_batch) that need no device, as a stand-alone program
// (tests/test_g16_batch_host.py builds it with g++, plain and with -fsanitize=address,undefined, and runs it):
//   (a) the group rule, the scratch layout and the argument checks of kogarashi_amd/csrc/groth16_batch.h
//   (b) the chain g16_mul2 and the assembly formulas of kogarashi_amd/csrc/groth16_assemble.h -- what the three assembly kernels run -- over
//       the device's field type, over the bound-tracking type of fp29_checked.h (it aborts when a column, limb or value bound of fp29.h
//       could be exceeded: 255 chained steps are machine-checked) and over the host's type of host_fp.h, each against a plain bit-by-bit
//       double-and-add written here.
// Prints "<checks> checks, <failures> failures"; the exit status is 0 only without failures.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/fp29_checked.h"
#include "../../kogarashi_amd/csrc/host_fp.h"
#include "../../kogarashi_amd/csrc/groth16_assemble.h"
#include "../../kogarashi_amd/csrc/groth16_batch.h"

using namespace kg;

static long g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// ---- (a) the group rule ----------------------------------------------------------------------------------------------------------------
static void group_rule() {
  CHECK(g16_batch_domain(1) == 2 && g16_batch_domain(2) == 2 && g16_batch_domain(3) == 4 && g16_batch_domain(16) == 16 && g16_batch_domain(17) == 32);
  CHECK(g16_batch_log(1) == 1 && g16_batch_log(2) == 1 && g16_batch_log(5) == 3 && g16_batch_log(1024) == 10 && g16_batch_log(1025) == 11);
  CHECK(g16_batch_domain((size_t)1 << 28) == (size_t)1 << 28 && g16_batch_log((size_t)1 << 28) == 28);
  CHECK(g16_batch_cap_bytes(256) == (size_t)256 << 20 && g16_batch_cap_bytes(0) == (size_t)1 << 20 && g16_batch_cap_bytes(-7) == (size_t)1 << 20);
  CHECK(g16_batch_cap_bytes(4096) == (size_t)4096 << 20 && g16_batch_cap_bytes(5000) == (size_t)4096 << 20);
  auto all_ok = [](int, size_t) { return true; };
  auto upto2048 = [](int, size_t len) { return len <= 2048; };
  for (size_t m : {(size_t)1, (size_t)2, (size_t)5, (size_t)16, (size_t)100, (size_t)1024, (size_t)2046}) {
    const size_t l = 2, w = m, n = g16_batch_domain(m), pb = g16_batch_proof_bytes(m, l, w);
    CHECK(pb == (3 * n + l + w) * 32 + 1024 && pb % 32 == 0);
    for (int mb : {1, 7, 256, 4096}) {
      const size_t cap = (size_t)mb << 20;
      for (size_t count : {(size_t)1, (size_t)2, (size_t)16, (size_t)1000, (size_t)1000003}) {
        size_t per = 99;
        const size_t groups = g16_batch_plan(m, l, w, count, mb, upto2048, &per);
        const size_t want_per = cap / pb < 1 ? 1 : (cap / pb < count ? cap / pb : count);
        CHECK(per == want_per && groups == (count + per - 1) / per);
        CHECK(per == 1 || per * pb <= cap);
        size_t next = 0;
        for (size_t g = 0; g < groups; ++g) {                          // the groups cover [0, count) exactly, in order, none empty, none too long
          const G16BatchGroup grp = g16_batch_group(per, count, g);
          CHECK(grp.first == next && grp.count >= 1 && grp.count <= per);
          next = grp.first + grp.count;
        }
        CHECK(next == count);
      }
    }
    // the layout: arrays in order, none overlapping, all inside the group's bytes, 16-byte aligned where 16-byte loads read them
    for (size_t g : {(size_t)1, (size_t)7, (size_t)130}) {
      const G16BatchLayout L = g16_batch_layout(g, n, l + w);
      CHECK(L.poly == 0 && L.z == 3 * g * n * 32 && L.sa == L.z + g * (l + w) * 32);
      CHECK(L.sb1 - L.sa == g * 64 && L.sl - L.sb1 == g * 64 && L.sh - L.sl == g * 64 && L.sb2 - L.sh == g * 64 && L.chains - L.sb2 == g * 128);
      CHECK(L.flags - L.chains == g * 4 * 36 * 4 && L.flags + 5 * g <= L.bytes && L.bytes == g * pb);
      CHECK(L.z % 32 == 0 && L.sa % 32 == 0 && L.sb2 % 16 == 0 && L.chains % 4 == 0);
    }
  }
  size_t per = 99;
  CHECK(g16_batch_plan(1024, 2, 1024, 16, 1, upto2048, &per) == 3 && per == 7);                  // 1 MiB / 132160 bytes: groups of 7, 7, 2
  CHECK(g16_batch_plan(2046, 2, 2046, 4, 256, upto2048, &per) == 1 && per == 4);
  CHECK(g16_batch_plan(2047, 2, 2047, 4, 256, upto2048, &per) == 0 && per == 0);                 // 2049 witness entries
  CHECK(g16_batch_plan(2050, 2, 100, 4, 256, upto2048, &per) == 0 && per == 0);                  // h's 2049 coefficients
  CHECK(g16_batch_plan(100, 2, 2049, 4, 256, upto2048, &per) == 0 && per == 0);                  // l's MSM
  CHECK(g16_batch_plan(16, 2, 16, 0, 256, all_ok, &per) == 0 && per == 0);                       // an empty batch
  CHECK(g16_batch_plan(0, 2, 16, 3, 256, all_ok, &per) == 0 && g16_batch_plan(16, 0, 16, 3, 256, all_ok, &per) == 0);
  CHECK(g16_batch_plan(((size_t)1 << 28) + 1, 2, 16, 3, 256, all_ok, &per) == 0 && g16_batch_plan(16, 2, SIZE_MAX / 2, 3, 256, all_ok, &per) == 0);
  CHECK(g16_batch_plan(16, 2, 16, 3, 256, all_ok, nullptr) == 1);                                // the out-pointer is optional
  CHECK(g16_batch_plan((size_t)1 << 28, 2, 16, 3, 256, all_ok, &per) == 3 && per == 1);          // a proof larger than the cap: one per group
  {                                                                                              // which lengths are asked for: zero lengths are not
    std::vector<std::pair<int, size_t>> asked;
    auto rec = [&asked](int curve, size_t len) { asked.push_back({curve, len}); return true; };
    CHECK(g16_batch_plan(1, 3, 0, 2, 256, rec, &per) == 1 && asked.size() == 2 && asked[0] == std::make_pair(0, (size_t)3) && asked[1] == std::make_pair(2, (size_t)3));
    asked.clear();
    CHECK(g16_batch_plan(9, 2, 9, 2, 256, rec, &per) == 1 && asked.size() == 4 && asked[2] == std::make_pair(0, (size_t)9) && asked[3] == std::make_pair(0, (size_t)8));
  }
  // the argument checks: nothing is dereferenced (the pointers are this frame's)
  int x = 0;
  const void* p = &x;
  CHECK(g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, 2, p, 5, p, p, 3, p, p) && g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 9, p, 4, p, 11, p, p, 3, p, p));
  CHECK(!g16_batch_args_ok(nullptr, p, 5, 2, 5, p, p, p, 5, p, 2, p, 5, p, p, 3, p, p) && !g16_batch_args_ok(p, nullptr, 5, 2, 5, p, p, p, 5, p, 2, p, 5, p, p, 3, p, p));
  for (int null_at = 0; null_at < 9; ++null_at) {                                                // every array, one at a time
    const void* a[9] = {p, p, p, p, p, p, p, p, p};
    a[null_at] = nullptr;
    CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, a[0], a[1], a[2], 5, a[3], 2, a[4], 5, a[5], a[6], 3, a[7], a[8]));
    CHECK(g16_batch_args_ok(p, p, 5, 2, 5, a[0], a[1], a[2], 5, a[3], 2, a[4], 5, a[5], a[6], 0, a[7], a[8]));       // count == 0: nothing is read or written
  }
  CHECK(g16_batch_args_ok(p, p, 5, 7, 0, p, p, p, 5, p, 7, nullptr, 0, p, p, 3, p, p));          // no witness values: w may be null
  CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 4, p, 2, p, 5, p, p, 3, p, p) && !g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, 1, p, 5, p, p, 3, p, p) &&
        !g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, 2, p, 4, p, p, 3, p, p));               // a stride shorter than its length
  CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 4, p, 2, p, 5, p, p, 0, p, p));               // ... also for an empty batch
  CHECK(!g16_batch_args_ok(p, p, 0, 2, 5, p, p, p, 5, p, 2, p, 5, p, p, 3, p, p) && !g16_batch_args_ok(p, p, 5, 0, 5, p, p, p, 5, p, 2, p, 5, p, p, 3, p, p));
  CHECK(!g16_batch_args_ok(p, p, ((size_t)1 << 28) + 1, 2, 5, p, p, p, (size_t)1 << 29, p, 2, p, 5, p, p, 3, p, p));
  CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, (size_t)1 << 60, p, 2, p, 5, p, p, 16, p, p));                        // count * eval_stride * 32 bytes
  CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, SIZE_MAX / 64 + 1, p, 5, p, p, 2, p, p) && g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, SIZE_MAX / 64, p, 5, p, p, 2, p, p));
  CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, 2, p, SIZE_MAX, p, p, 2, p, p));
  CHECK(!g16_batch_args_ok(p, p, 5, 2, 5, p, p, p, 5, p, 2, p, 5, p, p, SIZE_MAX / 256 + 1, p, p));                      // count proofs of 256 bytes
  CHECK(!g16_batch_args_ok(p, p, 5, 2, SIZE_MAX / 64 + 1, p, p, p, 5, p, 2, p, SIZE_MAX / 64 + 1, p, p, 1, p, p));         // (l + m_l_1) * 32
}

// ---- (b) the chain and the formulas -------------------------------------------------------------------------------------------------------
// ABI words (4 x u64 per base-field element, Montgomery R = 2^256) <-> a field type
template <class F> struct Io;
template <class P> struct Io<Fp<P>> {
  static constexpr int E = 4;
  static Fp<P> load(const uint64_t* w) { uint32_t v[8]; std::memcpy(v, w, 32); return from_ref<P>(v); }
  static void store(const Fp<P>& a, uint64_t* w) { uint32_t v[8]; to_ref(a, v); std::memcpy(w, v, 32); }
};
template <class P> struct Io<FpChecked<P>> {
  static constexpr int E = 4;
  static FpChecked<P> load(const uint64_t* w) {
    uint32_t v[8];
    std::memcpy(v, w, 32);
    return mul(FpChecked<P>::wrap(limbs_from_words<P>(v), 5.4), FpChecked<P>::from_const(P::C_FROM_REF));     // any 256-bit input
  }
  static void store(const FpChecked<P>& a, uint64_t* w) {
    uint32_t v[8];
    words_from_limbs(reduce_2p(mul(a, FpChecked<P>::from_const(P::C_TO_REF))).v, v);
    std::memcpy(w, v, 32);
  }
};
template <class P> struct Io<HostFp<P>> {
  static constexpr int E = 4;
  static HostFp<P> load(const uint64_t* w) { return HostFp<P>::from_words(w); }
  static void store(const HostFp<P>& a, uint64_t* w) { a.to_words(w); }
};
template <class G> struct Io<Fp2<G>> {
  static constexpr int E = 8;
  static Fp2<G> load(const uint64_t* w) { return {Io<G>::load(w), Io<G>::load(w + 4)}; }
  static void store(const Fp2<G>& a, uint64_t* w) { Io<G>::store(a.c0, w); Io<G>::store(a.c1, w + 4); }
};
// a point travels between the types as the device hands it on: affine ABI words and a flag
struct PointWords { uint64_t xy[16]; bool inf; };
template <class F> PointWords to_words(const XYZZ<F>& p) {
  PointWords r;
  std::memset(r.xy, 0, sizeof r.xy);
  Affine<F> a;
  r.inf = !to_affine(p, a);
  if (!r.inf) { Io<F>::store(a.x, r.xy); Io<F>::store(a.y, r.xy + Io<F>::E); }
  return r;
}
template <class F> XYZZ<F> from_words(const PointWords& w) {
  if (w.inf) return XYZZ<F>::identity();
  return from_affine(Affine<F>{Io<F>::load(w.xy), Io<F>::load(w.xy + Io<F>::E)});
}
static bool same(const PointWords& a, const PointWords& b) { return a.inf == b.inf && (a.inf || std::memcmp(a.xy, b.xy, sizeof a.xy) == 0); }

// a non-negative integer of up to 320 bits
struct Big {
  uint64_t l[5] = {0, 0, 0, 0, 0};
  void add_shifted(uint64_t d, int shift) {                    // += d * 2^shift
    unsigned __int128 carry = 0;
    const int j = shift >> 6, s = shift & 63;
    const uint64_t lo = d << s, hi = s ? d >> (64 - s) : 0;
    for (int i = j; i < 5; ++i) {
      const unsigned __int128 t = (unsigned __int128)l[i] + (i == j ? lo : (i == j + 1 ? hi : 0)) + carry;
      l[i] = (uint64_t)t;
      carry = t >> 64;
    }
  }
  void add_mul(const uint32_t k[8], uint32_t c) {              // += c * k
    for (int i = 0; i < 8; ++i) add_shifted((uint64_t)k[i] * c, 32 * i);
  }
  int bit(int i) const { return (int)((l[i >> 6] >> (i & 63)) & 1); }
};
// k * g by plain double-and-add, most significant bit first
template <class F> XYZZ<F> scalar_mul(const XYZZ<F>& g, const Big& k) {
  XYZZ<F> acc = XYZZ<F>::identity();
  for (int b = 319; b >= 0; --b) {
    acc = double_xyzz(acc);
    if (k.bit(b)) acc = add_xyzz(acc, g);
  }
  return acc;
}
template <class F> XYZZ<F> scalar_mul_words(const XYZZ<F>& g, const uint32_t k[8]) {
  Big b;
  b.add_mul(k, 1);
  return scalar_mul(g, b);
}
static Big small(uint64_t v) { Big b; b.add_shifted(v, 0); return b; }

// the generators as affine ABI words: G1 (1, 2), G2 (the twist's generator)
static PointWords gen_words(int curve) {
  PointWords r;
  std::memset(r.xy, 0, sizeof r.xy);
  r.inf = false;
  if (curve == 0) {
    uint32_t k1[8] = {1, 0, 0, 0, 0, 0, 0, 0}, k2[8] = {2, 0, 0, 0, 0, 0, 0, 0};
    Io<Fq>::store(from_int<FqParams>(k1), r.xy);
    Io<Fq>::store(from_int<FqParams>(k2), r.xy + 4);
    return r;
  }
  const uint32_t g2[4][8] = {{0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
                             {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
                             {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
                             {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};       // canonical integers
  for (int i = 0; i < 4; ++i) Io<Fq>::store(from_int<FqParams>(g2[i]), r.xy + 4 * i);
  return r;
}

// the scalars of the cases, canonical integers: 0, 1, r - 1 (the group's order minus one), 2^253, 2^254 - 1 (every bit set), two random ones
static const uint32_t K_ZERO[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static const uint32_t K_ONE[8] = {1, 0, 0, 0, 0, 0, 0, 0};
static const uint32_t K_RM1[8] = {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
static const uint32_t K_2_253[8] = {0, 0, 0, 0, 0, 0, 0, 0x20000000u};
static const uint32_t K_ONES[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};
static const uint32_t K_RND1[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 0x5cedc834u, 0x1082276bu, 0xf3a27251u, 0xf86c6a11u, 0x1d2c5e3fu};
static const uint32_t K_RND2[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x2be0cd19u};

// g16_mul2 over type T from the words of p and q
template <class T> PointWords chain_over(const PointWords& p, const uint32_t k1[8], const PointWords& q, const uint32_t k2[8]) {
  return to_words(g16_mul2<T>(from_words<T>(p), k1, from_words<T>(q), k2));
}
// One case: k1 p + k2 q by the chain over the three types against the plain double-and-add over FP
template <class FP, class FC, class FH>
static void chain_case(const PointWords& p, const uint32_t k1[8], const PointWords& q, const uint32_t k2[8], const char* what, int want_identity = -1) {
  const PointWords want = to_words(add_xyzz(scalar_mul_words(from_words<FP>(p), k1), scalar_mul_words(from_words<FP>(q), k2)));
  const PointWords got[3] = {chain_over<FP>(p, k1, q, k2), chain_over<FC>(p, k1, q, k2), chain_over<FH>(p, k1, q, k2)};
  for (int t = 0; t < 3; ++t) {
    ++g_checks;
    if (!same(got[t], want) || (want_identity >= 0 && (int)want.inf != want_identity)) {
      ++g_fail;
      std::fprintf(stderr, "FAILED chain: type %d (%s)\n", t, what);
    }
  }
}

template <class FP, class FC, class FH>
static void chain_cases(int curve) {
  const XYZZ<FP> G = from_words<FP>(gen_words(curve));
  const PointWords P = to_words(scalar_mul(G, small(5))), Q = to_words(scalar_mul(G, small(7))), NP = to_words(neg_xyzz(from_words<FP>(P)));
  PointWords ID = P;
  ID.inf = true;
  const uint32_t* ks[7] = {K_ZERO, K_ONE, K_RM1, K_2_253, K_ONES, K_RND1, K_RND2};
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) {
      if (curve == 2 && i >= 2 && j >= 2 && i != j && !(i == 5 && j == 6)) continue;          // G2: the edge rows and the diagonal (time)
      chain_case<FP, FC, FH>(P, ks[i], Q, ks[j], "two points");
    }
  for (int i = 0; i < 7; ++i) chain_case<FP, FC, FH>(P, ks[i], ID, K_ZERO, "one point, the second operand absent (roles 0, 1, 4)");
  chain_case<FP, FC, FH>(P, K_ZERO, Q, K_ZERO, "both scalars zero: the identity", 1);
  chain_case<FP, FC, FH>(P, K_RND1, NP, K_RND1, "q = -p with k1 = k2: the identity", 1);
  chain_case<FP, FC, FH>(P, K_ONES, NP, K_ONES, "q = -p, every bit set: the identity", 1);
  chain_case<FP, FC, FH>(P, K_RND1, NP, K_RND2, "q = -p, different scalars");
  chain_case<FP, FC, FH>(P, K_RND1, P, K_RND2, "p = q: p + q is a doubling");
  chain_case<FP, FC, FH>(P, K_ONES, P, K_ONES, "p = q, every bit set");
  chain_case<FP, FC, FH>(P, K_RM1, P, K_ONE, "p = q with k1 + k2 = r: the identity at the last step", 1);
  chain_case<FP, FC, FH>(ID, K_RND1, Q, K_RND2, "p the identity (an empty sum Sa)");
  chain_case<FP, FC, FH>(ID, K_RND1, ID, K_RND2, "both the identity", 1);
}

// The formulas of a proof over type T, with every point a known multiple of the generator: delta = 23 G, alpha = 2 G, beta = 3 G,
// Sa = a G, Sb = 13 G, Sl = 17 G, Sh = 19 G (a < 0: Sa = -(alpha + r delta), which makes A the identity).
struct ProofWords { PointWords a, c; };
template <class T>
static ProofWords assemble_over(const PointWords& delta, const PointWords& alpha, const PointWords& beta, const PointWords& sa, const PointWords& sb, const PointWords& sl,
                                const PointWords& sh, const uint32_t r_ref[8], const uint32_t s_ref[8]) {
  uint32_t k1[8], k2[8];
  const XYZZ<T> id = XYZZ<T>::identity();
  g16_chain_scalars(G16_ROLE_R_DELTA, r_ref, s_ref, k1, k2);
  const XYZZ<T> c0 = g16_mul2<T>(from_words<T>(delta), k1, id, k2);
  g16_chain_scalars(G16_ROLE_RS_DELTA, r_ref, s_ref, k1, k2);
  const XYZZ<T> c1 = g16_mul2<T>(from_words<T>(delta), k1, id, k2);
  g16_chain_scalars(G16_ROLE_VK, r_ref, s_ref, k1, k2);
  const XYZZ<T> c2 = g16_mul2<T>(from_words<T>(alpha), k1, from_words<T>(beta), k2);
  g16_chain_scalars(G16_ROLE_SUMS, r_ref, s_ref, k1, k2);
  const XYZZ<T> c3 = g16_mul2<T>(from_words<T>(sa), k1, from_words<T>(sb), k2);
  return {to_words(g16_point_ab(c0, from_words<T>(alpha), from_words<T>(sa))), to_words(g16_point_c(c1, c2, c3, from_words<T>(sl), from_words<T>(sh)))};
}
template <class FP, class FC, class FH>
static void assembly_case(int curve, const uint32_t r_int[8], const uint32_t s_int[8], bool cancel_a, bool empty_sums, const char* what) {
  const XYZZ<FP> G = from_words<FP>(gen_words(curve));
  uint32_t r_ref[8], s_ref[8], rs_int[8], k2[8];
  int_to_ref<FrParams>(r_int, r_ref);
  int_to_ref<FrParams>(s_int, s_ref);
  g16_chain_scalars(G16_ROLE_RS_DELTA, r_ref, s_ref, rs_int, k2);               // r s mod the group order
  const PointWords delta = to_words(scalar_mul(G, small(23))), alpha = to_words(scalar_mul(G, small(2))), beta = to_words(scalar_mul(G, small(3)));
  PointWords sa = to_words(scalar_mul(G, small(11))), sb = to_words(scalar_mul(G, small(13))), sl = to_words(scalar_mul(G, small(17))), sh = to_words(scalar_mul(G, small(19)));
  Big ka, kc;                                                             // A = ka G, C = kc G by integers
  ka.add_mul(r_int, 23); ka.add_shifted(2, 0);
  kc.add_mul(rs_int, 23); kc.add_mul(s_int, 2); kc.add_mul(r_int, 3);
  if (empty_sums) { sa.inf = sb.inf = sl.inf = sh.inf = true; }
  else if (cancel_a) {
    sa = to_words(neg_xyzz(scalar_mul(G, ka)));                                  // Sa = -(alpha + r delta)
    kc = Big(); kc.add_mul(r_int, 3 + 13); kc.add_shifted(17 + 19, 0);           // s Sa = -(23 r s + 2 s) G: what is left of C is (3 + 13) r + 17 + 19
    ka = Big();
  } else {
    ka.add_shifted(11, 0);
    kc.add_mul(s_int, 11); kc.add_mul(r_int, 13); kc.add_shifted(17 + 19, 0);
  }
  const PointWords want_a = to_words(scalar_mul(G, ka)), want_c = to_words(scalar_mul(G, kc));
  const ProofWords got[3] = {assemble_over<FP>(delta, alpha, beta, sa, sb, sl, sh, r_ref, s_ref), assemble_over<FC>(delta, alpha, beta, sa, sb, sl, sh, r_ref, s_ref),
                             assemble_over<FH>(delta, alpha, beta, sa, sb, sl, sh, r_ref, s_ref)};
  for (int t = 0; t < 3; ++t) {
    ++g_checks;
    if (!same(got[t].a, want_a) || !same(got[t].c, want_c) || (cancel_a && !got[t].a.inf)) {
      ++g_fail;
      std::fprintf(stderr, "FAILED assembly: curve %d type %d (%s)\n", curve, t, what);
    }
  }
}
template <class FP, class FC, class FH>
static void assembly_cases(int curve) {
  assembly_case<FP, FC, FH>(curve, K_RND1, K_RND2, false, false, "ordinary");
  assembly_case<FP, FC, FH>(curve, K_RND1, K_RND2, true, false, "Sa = -(alpha + r delta): A is the identity");
  assembly_case<FP, FC, FH>(curve, K_RND2, K_RND1, false, true, "every sum the identity");
  assembly_case<FP, FC, FH>(curve, K_ZERO, K_ZERO, false, false, "r = s = 0: no blinding");
  assembly_case<FP, FC, FH>(curve, K_ZERO, K_RND1, false, false, "r = 0");
  assembly_case<FP, FC, FH>(curve, K_RM1, K_ZERO, false, false, "r = p - 1, s = 0");
  assembly_case<FP, FC, FH>(curve, K_RM1, K_RM1, false, false, "r = s = p - 1: r s = 1");
  assembly_case<FP, FC, FH>(curve, K_ONE, K_2_253, true, false, "r = 1, s = 2^253, A the identity");
}

// the scalars of the roles from Montgomery words
static void role_scalars() {
  const uint32_t three[8] = {3, 0, 0, 0, 0, 0, 0, 0}, five[8] = {5, 0, 0, 0, 0, 0, 0, 0}, fifteen[8] = {15, 0, 0, 0, 0, 0, 0, 0};
  uint32_t r_ref[8], s_ref[8], k1[8], k2[8];
  int_to_ref<FrParams>(three, r_ref);
  int_to_ref<FrParams>(five, s_ref);
  g16_chain_scalars(G16_ROLE_R_DELTA, r_ref, s_ref, k1, k2);
  CHECK(std::memcmp(k1, three, 32) == 0 && std::memcmp(k2, K_ZERO, 32) == 0);
  g16_chain_scalars(G16_ROLE_RS_DELTA, r_ref, s_ref, k1, k2);
  CHECK(std::memcmp(k1, fifteen, 32) == 0 && std::memcmp(k2, K_ZERO, 32) == 0);
  for (int role : {G16_ROLE_VK, G16_ROLE_SUMS}) {
    g16_chain_scalars(role, r_ref, s_ref, k1, k2);
    CHECK(std::memcmp(k1, five, 32) == 0 && std::memcmp(k2, three, 32) == 0);
  }
  g16_chain_scalars(G16_ROLE_G2, r_ref, s_ref, k1, k2);
  CHECK(std::memcmp(k1, five, 32) == 0 && std::memcmp(k2, K_ZERO, 32) == 0);
  int_to_ref<FrParams>(K_RM1, r_ref);
  g16_chain_scalars(G16_ROLE_RS_DELTA, r_ref, r_ref, k1, k2);                   // (p - 1)^2 = 1
  CHECK(std::memcmp(k1, K_ONE, 32) == 0);
  g16_chain_scalars(G16_ROLE_R_DELTA, r_ref, r_ref, k1, k2);
  CHECK(std::memcmp(k1, K_RM1, 32) == 0);
}

int main() {
  group_rule();
  role_scalars();
  chain_cases<Fq, FqC, HostFq>(0);
  chain_cases<Fq2, Fq2C, HostFq2>(2);
  assembly_cases<Fq, FqC, HostFq>(0);
  assembly_cases<Fq2, Fq2C, HostFq2>(2);
  std::printf("%ld checks, %ld failures\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
