// msm_batch_host.cpp -- the parts of the batched short MSM (kg_commit_batch) that need no device, as a stand-alone program
// (tests/test_msm_batch_host.py builds it with g++, plain and with -fsanitize=address,undefined, and runs it):
//   (a) the launch-group rule and the argument checks of kogarashi_amd/csrc/msm_small_batch.h
//   (b) the finish chain of kogarashi_amd/csrc/msm_small_finish.h -- what k_small_finish_batch runs with one lane per vector -- over the
//       device's field type, over the bound-tracking type of fp29_checked.h (it aborts when a column, limb or value bound of fp29.h could be
//       exceeded) and over the host's type of host_fp.h (the chain kg_commit finishes with), from the same ABI words the device reads.
// Prints "<checks> checks, <failures> failures"; the exit status is 0 only without failures.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/fp29_checked.h"
#include "../../kogarashi_amd/csrc/host_fp.h"
#include "../../kogarashi_amd/csrc/msm_small_finish.h"
#include "../../kogarashi_amd/csrc/msm_small_batch.h"

using namespace kg;

static long g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// ---- (a) the group rule ----------------------------------------------------------------------------------------------------------------
static void group_rule() {
  const int widths[] = {2, 3, 4, 5, 6, 8, 10};
  for (int curve = 0; curve < 3; ++curve)
    for (int c : widths)
      for (int r = 0; r <= c - 1 && r <= 7; ++r)
        for (int glv = 0; glv < 2; ++glv) {
          if (c - 1 - r > 5) continue;                                   // at most 32 workgroups per window (msm_small_plan)
          const MsmBatchShape sh{curve, c, r, glv != 0, 100};
          const size_t W = (size_t)msm_batch_windows(sh), NB = (size_t)msm_batch_ranges(sh), E = curve == 2 ? 8 : 4, NW = curve == 2 ? 72 : 36;
          CHECK(W == (size_t)((glv ? 128 : 255) + c - 1) / c && NB == (size_t)1 << (c - 1 - r));
          CHECK(msm_batch_sums_bytes(sh) == W * 4 * E * 8);
          CHECK(msm_batch_planes_bytes(sh) == (NB > 1 ? W * NB * 8 * NW * 4 : 0));
          const size_t vb = msm_batch_vector_bytes(sh), per = msm_batch_per_launch(vb);
          CHECK(vb == msm_batch_sums_bytes(sh) + msm_batch_planes_bytes(sh) && vb % 16 == 0);
          CHECK(per >= 1 && per <= 65535 && per <= MSM_BATCH_GRID_MAX);
          CHECK(per * vb <= MSM_BATCH_SCRATCH_CAP);
          CHECK(per == 65535 || (per + 1) * vb > MSM_BATCH_SCRATCH_CAP);   // the most the cap admits
          for (size_t count : {(size_t)0, (size_t)1, per - 1, per, per + 1, 2 * per, 2 * per + 1, (size_t)1000003}) {
            const size_t groups = msm_batch_groups(per, count);
            CHECK(groups == (count + per - 1) / per);
            size_t next = 0;
            for (size_t g = 0; g < groups; ++g) {                          // the groups cover [0, count) exactly, in order, none empty, none too long
              const MsmBatchGroup grp = msm_batch_group(per, count, g);
              CHECK(grp.first == next && grp.count >= 1 && grp.count <= per);
              next = grp.first + grp.count;
            }
            CHECK(next == count);
            CHECK(msm_batch_scratch_bytes(vb, count) == (count < per ? count : per) * vb && msm_batch_scratch_bytes(vb, count) <= MSM_BATCH_SCRATCH_CAP);
          }
        }
  // empty vectors: no windows, no scratch, the grid's limit alone
  const MsmBatchShape empty{0, 0, 0, false, 0};
  CHECK(msm_batch_windows(empty) == 0 && msm_batch_ranges(empty) == 1 && msm_batch_vector_bytes(empty) == 0);
  CHECK(msm_batch_per_launch(0) == 65535 && msm_batch_groups(65535, 65536) == 2 && msm_batch_scratch_bytes(0, 70000) == 0);
  CHECK(msm_batch_per_launch(MSM_BATCH_SCRATCH_CAP) == 1 && msm_batch_per_launch(MSM_BATCH_SCRATCH_CAP + 1) == 1 && msm_batch_per_launch(SIZE_MAX) == 1);
  CHECK(msm_batch_per_launch(1024) == 65535 && msm_batch_per_launch(1025) == MSM_BATCH_SCRATCH_CAP / 1025);
  CHECK(msm_batch_groups(0, 5) == 0 && msm_batch_groups(7, 0) == 0);
  // the argument checks: nothing is dereferenced (the pointers are this frame's)
  int x = 0;
  const void* p = &x;
  CHECK(msm_batch_args_ok(p, 0, p, p, 4, 3, 4, p, p) && msm_batch_args_ok(p, 2, p, p, 4, 3, 9, p, p) && msm_batch_args_ok(p, 1, p, p, 1, 1, 1, p, p));
  CHECK(!msm_batch_args_ok(nullptr, 0, p, p, 4, 3, 4, p, p));                            // null context
  CHECK(!msm_batch_args_ok(p, 0, nullptr, p, 4, 3, 4, p, p) && !msm_batch_args_ok(p, 0, p, nullptr, 4, 3, 4, p, p));      // null inputs where pairs are read
  CHECK(!msm_batch_args_ok(p, 0, p, p, 4, 3, 4, nullptr, p) && !msm_batch_args_ok(p, 0, p, p, 4, 3, 4, p, nullptr));      // null outputs
  CHECK(!msm_batch_args_ok(p, 0, p, p, 4, 3, 3, p, p));                                  // stride < n
  CHECK(!msm_batch_args_ok(p, -1, p, p, 4, 3, 4, p, p) && !msm_batch_args_ok(p, 3, p, p, 4, 3, 4, p, p));               // unknown curve
  CHECK(msm_batch_args_ok(p, 0, nullptr, nullptr, 0, 3, 0, p, p) && !msm_batch_args_ok(p, 0, nullptr, nullptr, 0, 3, 0, nullptr, p));   // n == 0: identities are written
  CHECK(msm_batch_args_ok(p, 0, nullptr, nullptr, 4, 0, 4, nullptr, nullptr) && !msm_batch_args_ok(p, 0, nullptr, nullptr, 4, 0, 3, nullptr, nullptr));   // count == 0
  CHECK(!msm_batch_args_ok(p, 0, p, p, 4, (size_t)1 << 60, 16, p, p));                   // count * stride * 32 bytes overflow
  CHECK(!msm_batch_args_ok(p, 0, p, p, 4, 2, SIZE_MAX, p, p) && !msm_batch_args_ok(p, 0, p, p, 4, 2, SIZE_MAX / 64 + 1, p, p));
  CHECK(msm_batch_args_ok(p, 0, p, p, 4, 2, SIZE_MAX / 64, p, p));
  CHECK(!msm_batch_args_ok(p, 2, p, p, 0, SIZE_MAX / 128 + 1, 0, p, p) && !msm_batch_args_ok(p, 0, p, p, 0, SIZE_MAX / 64 + 1, 0, p, p));   // count points
  CHECK(!msm_batch_args_ok(p, 2, p, p, SIZE_MAX / 128 + 1, 1, SIZE_MAX / 128 + 1, p, p));                                   // n bases
}

// ---- (b) the finish chain --------------------------------------------------------------------------------------------------------------
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
template <class F> XYZZ<F> load_point(const uint64_t* w) {
  constexpr int E = Io<F>::E;
  return {Io<F>::load(w), Io<F>::load(w + E), Io<F>::load(w + 2 * E), Io<F>::load(w + 3 * E)};
}
template <class F> void store_point(const XYZZ<F>& p, uint64_t* w) {
  constexpr int E = Io<F>::E;
  Io<F>::store(p.x, w); Io<F>::store(p.y, w + E); Io<F>::store(p.zz, w + 2 * E); Io<F>::store(p.zzz, w + 3 * E);
}

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

// the generators as affine ABI words: G1 (1, 2), Grumpkin (1, sqrt(-16)), G2 (the twist's generator)
static void gen_words(int curve, uint64_t* xy) {
  auto from_small = [](auto tag, uint32_t v, uint64_t* w) {
    using P = decltype(tag);
    uint32_t k[8] = {v, 0, 0, 0, 0, 0, 0, 0};
    Io<Fp<P>>::store(from_int<P>(k), w);
  };
  if (curve == 0) { from_small(FqParams{}, 1, xy); from_small(FqParams{}, 2, xy + 4); return; }
  if (curve == 1) {
    from_small(FrParams{}, 1, xy);
    const uint32_t y[8] = {0x448c41d8u, 0x11b2dff1u, 0x21c77dc3u, 0x23d3446fu, 0x35dfafbbu, 0xaa7b8cf4u, 0x9dc25d68u, 0x14b34cf6u};      // ABI form
    std::memcpy(xy + 4, y, 32);
    return;
  }
  const uint32_t g2[4][8] = {{0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
                             {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
                             {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
                             {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};       // canonical integers
  for (int i = 0; i < 4; ++i) Io<Fq>::store(from_int<FqParams>(g2[i]), xy + 4 * i);
}

// chain over type F from the ABI words of the window sums; returns false for the identity
template <class F> bool run_chain(const std::vector<uint64_t>& sums, int W, int c, uint64_t* xy) {
  constexpr int E = Io<F>::E;
  Affine<F> a;
  const uint64_t* base = sums.data();
  if (!small_finish_affine<F>(W, c, [base](int w) { return load_point<F>(base + (size_t)w * 4 * E); }, a)) return false;
  Io<F>::store(a.x, xy); Io<F>::store(a.y, xy + E);
  return true;
}

// One case: window sums S_w = d[w] * G (negative d: the negated point), built in the device's type FP and exported as the device exports them;
// the chain over FP, the checked type FC and the host's type FH must give sum_w d[w] 2^(c w) * G by plain double-and-add, bit for bit.
template <class FP, class FC, class FH>
static void chain_case(int curve, int c, int W, const std::vector<long long>& d, const char* what) {
  constexpr int E = Io<FP>::E;
  uint64_t gw[16];
  gen_words(curve, gw);
  const XYZZ<FP> G = from_affine(Affine<FP>{Io<FP>::load(gw), Io<FP>::load(gw + E)});
  std::vector<uint64_t> sums((size_t)W * 4 * E);
  Big pos, neg;
  for (int w = 0; w < W; ++w) {
    Big k;
    const unsigned long long m = (unsigned long long)(d[w] < 0 ? -d[w] : d[w]);
    k.add_shifted(m, 0);
    XYZZ<FP> s = scalar_mul(G, k);
    if (d[w] < 0) s = neg_xyzz(s);
    store_point(s, sums.data() + (size_t)w * 4 * E);
    (d[w] < 0 ? neg : pos).add_shifted(m, c * w);
  }
  const XYZZ<FP> want_p = add_xyzz(scalar_mul(G, pos), neg_xyzz(scalar_mul(G, neg)));
  Affine<FP> wa;
  const bool want_finite = to_affine(want_p, wa);
  uint64_t want[16] = {0}, got[3][16] = {{0}};
  if (want_finite) { Io<FP>::store(wa.x, want); Io<FP>::store(wa.y, want + E); }
  const bool fin[3] = {run_chain<FP>(sums, W, c, got[0]), run_chain<FC>(sums, W, c, got[1]), run_chain<FH>(sums, W, c, got[2])};
  for (int t = 0; t < 3; ++t) {
    ++g_checks;
    if (fin[t] != want_finite || (want_finite && std::memcmp(got[t], want, (size_t)2 * E * 8) != 0)) {
      ++g_fail;
      std::fprintf(stderr, "FAILED chain: curve %d c %d W %d type %d (%s)\n", curve, c, W, t, what);
    }
  }
}

template <class FP, class FC, class FH>
static void chain_cases(int curve) {
  uint64_t lcg = 0x9E3779B97F4A7C15ull + (uint64_t)curve;
  auto rnd = [&lcg](unsigned bits) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (long long)((lcg >> 33) & ((1ull << bits) - 1)); };
  for (int c : {2, 4, 5, 8})
    for (int bits : {128, 255}) {
      const int W = (bits + c - 1) / c;
      std::vector<long long> d(W), z(W, 0);
      for (int w = 0; w < W; ++w) d[w] = rnd(16);
      chain_case<FP, FC, FH>(curve, c, W, d, "known multiples in every window");
      for (int w = 0; w < W; ++w) d[w] = rnd((unsigned)c);               // what a window sum of unit bases would hold: digits below 2^c
      d[W / 2] = 0;
      chain_case<FP, FC, FH>(curve, c, W, d, "digit-sized multiples, one empty window");
      chain_case<FP, FC, FH>(curve, c, W, z, "every window sum the identity");
      std::vector<long long> t = z;
      t[W - 1] = 5;
      chain_case<FP, FC, FH>(curve, c, W, t, "only the top window");
      t = z; t[0] = 7;
      chain_case<FP, FC, FH>(curve, c, W, t, "only the bottom window");
      // S_w equal to the doubled accumulator: the addition meets an equal point (the doubling branch of add_xyzz), mid-chain and at the bottom
      for (int w = 0; w < W; ++w) d[w] = rnd(12);
      d[W - 1] = 3; d[W - 2] = 3ll << c;
      chain_case<FP, FC, FH>(curve, c, W, d, "a window sum equal to the doubled accumulator");
      t = z; t[1] = 9; t[0] = 9ll << c;
      chain_case<FP, FC, FH>(curve, c, W, t, "the bottom window sum equal to the doubled accumulator");
      // S_w equal to the negative of the doubled accumulator: the identity mid-chain (the chain goes on from it), and at the end
      d[W - 2] = -(3ll << c);
      chain_case<FP, FC, FH>(curve, c, W, d, "a window sum that cancels the accumulator mid-chain");
      t[0] = -(9ll << c);
      chain_case<FP, FC, FH>(curve, c, W, t, "the bottom window sum cancels the accumulator: the identity");
    }
}

int main() {
  group_rule();
  chain_cases<Fq, FqC, HostFq>(0);
  chain_cases<Fr, FrC, HostFr>(1);
  chain_cases<Fq2, Fq2C, HostFq2>(2);
  std::printf("%ld checks, %ld failures\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
