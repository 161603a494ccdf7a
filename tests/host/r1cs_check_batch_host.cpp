// r1cs_check_batch_host.cpp -- the parts of kg_r1cs_check_batch / kg_groth16_witness_check_batch (kogarashi_amd/csrc/vec.hip CheckOp) that
// need no device, as a stand-alone program: tests/test_r1cs_check_batch_host.py builds it with g++, plain and with -fsanitize=address,undefined,
// and runs it.
//
//   r1cs_check_batch_host            every section; prints one "ok: ..." line per section, exits non-zero at the first failure
//
//   args    r1cs_check_batch_args_ok / g16_witness_check_batch_args_ok (r1cs_batch.h, the header alone): every refusal and every accepted
//           empty case of the two entries
//   u       u_factor (vecops.h: the device's scaling of a vector's u) against u_scaled_words (what vec.hip's scaled() runs on the host) for
//           u in {0, 1, p - 1, random} over both fields, on the device type and on the bound-checked type; the checked value is then handed to
//           sat_residual_row, which aborts if it is not the factor form that function accepts
//   split   r1cs_split_at: column j of x || w at j in {0, l - 1, l, l + m_l_1 - 1}, with l = 1 and with m_l_1 = 0
//   fold    the walker's reporting over a simulated grid -- a lane per (row, vector) folded per wave as summary_fold does, the chunk rule
//           and the pointer offsets check_enqueue applies per chunk: vector b's pair and bytes depend on vector b's rows only, the bytes
//           between two vectors' rows stay untouched
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/r1cs_batch.h"
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/vecops.h"
#include "../../kogarashi_amd/csrc/host_fp.h"
#ifndef KG_R1CS_HOST_PLAIN_ONLY
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
  const size_t big = (size_t)1 << 32;
  auto ok = [&](const void* ctx, int field, const Csr* a, const Csr* b, const Csr* c, size_t m, const void* z, size_t zs, size_t count, const void* e, size_t es,
                const void* st, size_t ss, const void* sum) { return r1cs_check_batch_args_ok(ctx, field, a, b, c, m, z, zs, count, e, es, st, ss, sum); };
  EXPECT(ok(p, 0, &full, &full, &full, 5, p, 9, 3, p, 5, p, 5, p));                  // everything given
  EXPECT(ok(p, 1, &full, &full, &full, 5, p, 9, 3, nullptr, 0, nullptr, 0, p));      // no E, no status: their strides are not looked at
  EXPECT(ok(p, 0, &full, &full, &full, 5, p, 0, 3, p, 7, p, 8, p));                  // z_stride is trusted (0: one vector count times)
  // the refusals
  EXPECT(!ok(nullptr, 0, &full, &full, &full, 5, p, 9, 3, p, 5, p, 5, p));           // a null ctx
  EXPECT(!ok(nullptr, 0, &full, &full, &full, 0, p, 9, 0, p, 5, p, 5, p));           //   even for an empty call
  EXPECT(!ok(p, 2, &full, &full, &full, 5, p, 9, 3, p, 5, p, 5, p));                 // an unknown field
  EXPECT(!ok(p, -1, &full, &full, &full, 5, p, 9, 0, p, 5, p, 5, p));                //   even for an empty call
  EXPECT(!ok(p, 0, &full, &full, &full, big, p, 9, 3, nullptr, 0, nullptr, 0, p));   // m >= 2^32
  EXPECT(!ok(p, 0, &full, &full, &full, big, p, 9, 0, nullptr, 0, nullptr, 0, p));   //   even for an empty call
  EXPECT(ok(p, 0, &full, &full, &full, big - 1, p, 9, 3, nullptr, 0, nullptr, 0, p));
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, 9, 3, p, 5, p, 5, nullptr));           // a null d_summary with count > 0
  EXPECT(!ok(p, 0, &full, &full, &full, 0, p, 9, 3, p, 5, p, 5, nullptr));           //   also with m == 0: the pairs are written
  EXPECT(!ok(p, 0, nullptr, &full, &full, 5, p, 9, 3, p, 5, p, 5, p));               // a null kg_csr, each position
  EXPECT(!ok(p, 0, &full, nullptr, &full, 5, p, 9, 3, p, 5, p, 5, p));
  EXPECT(!ok(p, 0, &full, &full, nullptr, 5, p, 9, 3, p, 5, p, 5, p));
  EXPECT(!ok(p, 0, &no_rows, &full, &full, 5, p, 9, 3, p, 5, p, 5, p));              // a null member array, each member
  EXPECT(!ok(p, 0, &full, &no_col, &full, 5, p, 9, 3, p, 5, p, 5, p));
  EXPECT(!ok(p, 0, &full, &full, &no_val, 5, p, 9, 3, p, 5, p, 5, p));
  EXPECT(!ok(p, 0, &full, &full, &full, 5, nullptr, 9, 3, p, 5, p, 5, p));           // a null d_z
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, 9, 3, p, 4, p, 5, p));                 // e_stride < m with d_e given
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, 9, 3, p, 5, p, 4, p));                 // status_stride < m with d_status given
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, SIZE_MAX / 32 / 3 + 1, 3, p, 5, p, 5, p));        // count * stride * 32 beyond size_t: z,
  EXPECT(ok(p, 0, &full, &full, &full, 5, p, SIZE_MAX / 32 / 3, 3, p, 5, p, 5, p));
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, 9, 3, p, SIZE_MAX / 32 / 3 + 1, p, 5, p));        // E,
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, 9, 3, p, 5, p, SIZE_MAX / 3 + 1, p));             // the status bytes,
  EXPECT(!ok(p, 0, &full, &full, &full, 5, p, 9, SIZE_MAX / 8 + 1, nullptr, 0, nullptr, 0, p)); // the pairs themselves
  // the accepted empty cases
  EXPECT(ok(p, 0, nullptr, nullptr, nullptr, 5, nullptr, 0, 0, nullptr, 0, nullptr, 0, nullptr));      // count == 0: nothing is looked at,
  EXPECT(ok(p, 1, &no_rows, nullptr, &full, 5, nullptr, 0, 0, p, 1, p, 1, nullptr));                   //   short strides included
  EXPECT(ok(p, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 3, nullptr, 0, nullptr, 0, p));            // m == 0, count > 0: the pairs alone
  EXPECT(ok(p, 0, &no_val, &full, &full, 0, nullptr, 0, 3, p, 0, p, 0, p));

  auto wok = [&](const void* ctx, const Csr* a, const Csr* b, const Csr* c, size_t m, size_t l, size_t ml1, const void* x, size_t xs, const void* w, size_t ws,
                 size_t count, const void* st, size_t ss, const void* sum) { return g16_witness_check_batch_args_ok(ctx, a, b, c, m, l, ml1, x, xs, w, ws, count, st, ss, sum); };
  EXPECT(wok(p, &full, &full, &full, 5, 2, 6, p, 2, p, 6, 3, p, 5, p));
  EXPECT(wok(p, &full, &full, &full, 5, 2, 6, p, 4, p, 9, 3, nullptr, 0, p));        // wider strides, no status
  EXPECT(wok(p, &full, &full, &full, 5, 1, 0, p, 1, nullptr, 0, 3, p, 5, p));        // l = 1, no witness wire: d_w may be null
  EXPECT(wok(p, &full, &full, &full, 2047, 2, 2046, p, 2, p, 2046, 3, p, 2047, p));  // not bound to the batched MSM's 2048 pairs
  EXPECT(wok(p, &full, &full, &full, 1 << 20, 2, 1 << 20, p, 2, p, 1 << 20, 3, nullptr, 0, p));
  EXPECT(!wok(nullptr, &full, &full, &full, 5, 2, 6, p, 2, p, 6, 3, p, 5, p));       // a null ctx
  EXPECT(!wok(p, &full, &full, &full, big, 2, 6, p, 2, p, 6, 3, nullptr, 0, p));     // m >= 2^32
  EXPECT(!wok(p, &full, &full, &full, 5, 0, 6, p, 2, p, 6, 3, p, 5, p));             // l < 1
  EXPECT(!wok(p, &full, &full, &full, 5, 0, 6, p, 2, p, 6, 0, p, 5, p));             //   even for an empty call
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, 1, p, 6, 3, p, 5, p));             // x_stride < l
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, 2, p, 5, 3, p, 5, p));             // w_stride < m_l_1
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, 2, p, 6, 3, p, 5, nullptr));       // a null d_summary with count > 0
  EXPECT(!wok(p, nullptr, &full, &full, 5, 2, 6, p, 2, p, 6, 3, p, 5, p));           // a null kg_csr
  EXPECT(!wok(p, &full, &no_col, &full, 5, 2, 6, p, 2, p, 6, 3, p, 5, p));           // a null member array
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, nullptr, 2, p, 6, 3, p, 5, p));       // a null d_x
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, 2, nullptr, 6, 3, p, 5, p));       // a null d_w with witness wires
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, 2, p, 6, 3, p, 4, p));             // status_stride < m with d_status given
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, SIZE_MAX / 32 / 3 + 1, p, 6, 3, p, 5, p));    // count * stride * 32 beyond size_t
  EXPECT(!wok(p, &full, &full, &full, 5, 2, 6, p, 2, p, SIZE_MAX / 32 / 3 + 1, 3, p, 5, p));
  EXPECT(wok(p, nullptr, nullptr, nullptr, 5, 2, 6, nullptr, 2, nullptr, 6, 0, nullptr, 0, nullptr));  // count == 0
  EXPECT(wok(p, nullptr, nullptr, nullptr, 0, 2, 6, nullptr, 2, nullptr, 6, 3, nullptr, 0, p));        // m == 0, count > 0
  if (!failures) std::printf("ok: args\n");
}

// ---- u --------------------------------------------------------------------------------------------------------------------------------
template <class F> struct RawIn;
template <class P> struct RawIn<Fp<P>> {
  static Fp<P> in(const uint32_t* w) { return limbs_from_words<P>(w); }
  static const Fp<P>& plain(const Fp<P>& x) { return x; }
};
#ifndef KG_R1CS_HOST_PLAIN_ONLY
template <class P> struct RawIn<FpChecked<P>> {
  static FpChecked<P> in(const uint32_t* w) { return FpChecked<P>::wrap(limbs_from_words<P>(w), 5.4); }      // any 256-bit input
  static const Fp<P>& plain(const FpChecked<P>& x) { return x.v; }
};
#endif

template <class F, class HostP>
static void u_cases(const char* what) {
  using P = typename F::Params;
  using H = HostFp<HostP>;
  const H one = H::one(), zero = H::zero(), minus_one = sub<4, 1>(zero, one);
  H rnd = one;                                             // a few values off a fixed chain: ((... * 7 + 1)^2 ...)
  std::vector<H> us = {zero, one, minus_one};
  for (int i = 0; i < 5; ++i) {
    for (int k = 0; k < 3; ++k) rnd = add(dbl(rnd), add(rnd, one));
    rnd = sqr(rnd);
    us.push_back(rnd);
    us.push_back(sub<4, 1>(zero, rnd));
  }
  for (const H& u : us) {
    uint64_t want[4];
    u_scaled_words<HostP>(u.v, want);                      // the host's ten doublings
    uint32_t wu[8], got[8], ww[8];
    std::memcpy(wu, u.v, 32);
    std::memcpy(ww, want, 32);
    const F us_dev = u_factor(RawIn<F>::in(wu), F::from_const(P::C_XT_U));
    words_from_limbs(RawIn<F>::plain(reduce_2p(us_dev)), got);
    if (std::memcmp(got, ww, 32) != 0) { std::fprintf(stderr, "%s: u_factor differs from the host's scaling\n", what); ++failures; }
    // the value as sat_residual_row takes it (the checked type aborts if it is not the factor form that function accepts); an empty row with
    // E = 0 holds whatever u is
    EXPECT(is_zero_mod_p(sat_residual_row(F::zero(), F::zero(), F::zero(), us_dev, F::zero(), F::from_const(P::C_XT_HAD))));
    // and a row with A z = B z = 0, C z = z0 * v0: the residual -u c - E vanishes for E = -u c and for no other E (E + 1 here)
    const H z0 = us[4], v0 = us[5], c_abi = mul(z0, v0), e_fit = sub<4, 1>(zero, mul(u, c_abi)), e_off = add(e_fit, one);
    uint32_t wz[8], wv[8], we[8];
    std::memcpy(wz, z0.v, 32);
    std::memcpy(wv, v0.v, 32);
    const F cz = dot_step(F::zero(), RawIn<F>::in(wz), RawIn<F>::in(wv));
    std::memcpy(we, e_fit.v, 32);
    EXPECT(is_zero_mod_p(sat_residual_row(F::zero(), F::zero(), cz, us_dev, RawIn<F>::in(we), F::from_const(P::C_XT_HAD))));
    std::memcpy(we, e_off.v, 32);
    EXPECT(!is_zero_mod_p(sat_residual_row(F::zero(), F::zero(), cz, us_dev, RawIn<F>::in(we), F::from_const(P::C_XT_HAD))));
  }
  if (!failures) std::printf("ok: u %s\n", what);
}

// ---- split ----------------------------------------------------------------------------------------------------------------------------
static void test_split() {
  struct { size_t l, ml1; } shapes[] = {{3, 5}, {1, 4}, {1, 0}, {4, 0}, {2, 2046}};
  for (auto s : shapes) {
    const size_t l = s.l, n = s.l + s.ml1;
    for (size_t j : {(size_t)0, l - 1, l, n - 1}) {
      if (j >= n) continue;                                // m_l_1 == 0: column l does not exist
      const R1csSplitAt at = r1cs_split_at(j, l);
      EXPECT(at.in_x == (j < l));
      EXPECT(at.index == (j < l ? j : j - l));
      EXPECT(at.in_x ? at.index < l : at.index < s.ml1);   // inside the array it selects
    }
    // the whole of x || w, in order, each element once
    std::vector<int> seen_x(l, 0), seen_w(s.ml1, 0);
    for (size_t j = 0; j < n; ++j) {
      const R1csSplitAt at = r1cs_split_at(j, l);
      ++(at.in_x ? seen_x : seen_w)[at.index];
    }
    for (int v : seen_x) EXPECT(v == 1);
    for (int v : seen_w) EXPECT(v == 1);
  }
  static_assert(r1cs_split_at(0, 1).in_x && r1cs_split_at(0, 1).index == 0, "l = 1: column 0 is x[0]");
  static_assert(!r1cs_split_at(1, 1).in_x && r1cs_split_at(1, 1).index == 0, "l = 1: column 1 is w[0]");
  if (!failures) std::printf("ok: split\n");
}

// ---- fold -----------------------------------------------------------------------------------------------------------------------------
// summary_add / summary_fold of common.h on the host: one speaker per wave, a count and a minimum
static void fold_wave(uint32_t* pair, const std::vector<uint8_t>& bad, size_t first_row) {
  uint32_t n = 0, lowest = 0;
  for (size_t k = bad.size(); k-- > 0;)
    if (bad[k]) { ++n; lowest = (uint32_t)(first_row + k); }
  if (n) { pair[0] += n; pair[1] = pair[1] < lowest ? pair[1] : lowest; }
}
static bool row_is_bad(size_t vec, size_t row) { return ((vec * 2654435761u + row * 40503u) >> 3) % 7 == 0 && vec % 5 != 1; }       // vectors 1, 6, ...: clean

static void simulate(size_t m, size_t count, size_t status_stride) {
  std::vector<uint32_t> sums(2 * count + 2, 0xA5A5A5A5u);
  std::vector<uint8_t> status(count * status_stride + 3, 0xA5);
  for (size_t b = 0; b < count; ++b) { sums[2 * b] = 0; sums[2 * b + 1] = (uint32_t)m; }       // k_check_batch_init
  size_t covered = 0;
  for (size_t i = 0; i < r1cs_batch_chunks(count); ++i) {
    const R1csBatchChunk ch = r1cs_batch_chunk(count, i);
    EXPECT(ch.first == covered && ch.count >= 1 && ch.count <= R1CS_BATCH_GRID_Y_MAX);
    covered += ch.count;
    uint32_t* chunk_sums = sums.data() + 2 * ch.first;                                        // the offsets check_enqueue applies
    uint8_t* chunk_status = status.data() + ch.first * status_stride;
    for (size_t y = 0; y < ch.count; ++y)                                                     // the grid's y
      for (size_t w0 = 0; w0 < m; w0 += 64) {                                                 // a wave of k_rows_lane: 64 rows of vector y
        std::vector<uint8_t> bad;
        for (size_t row = w0; row < w0 + 64 && row < m; ++row) {
          bad.push_back(row_is_bad(ch.first + y, row));
          chunk_status[r1cs_check_batch_status_byte(y, status_stride, row)] = bad.back();
        }
        fold_wave(chunk_sums + r1cs_check_batch_summary_word(y), bad, w0);
      }
  }
  EXPECT(covered == count);
  for (size_t b = 0; b < count; ++b) {                     // vector b's pair and bytes: from vector b's rows only
    uint32_t n = 0, first = (uint32_t)m;
    for (size_t row = m; row-- > 0;)
      if (row_is_bad(b, row)) { ++n; first = (uint32_t)row; }
    EXPECT(sums[2 * b] == n && sums[2 * b + 1] == first);
    for (size_t row = 0; row < m; ++row) EXPECT(status[b * status_stride + row] == (row_is_bad(b, row) ? 1 : 0));
    for (size_t k = m; k < status_stride; ++k) EXPECT(status[b * status_stride + k] == 0xA5);  // between two vectors' rows: untouched
  }
  EXPECT(sums[2 * count] == 0xA5A5A5A5u && sums[2 * count + 1] == 0xA5A5A5A5u);
  for (size_t k = 0; k < 3; ++k) EXPECT(status[count * status_stride + k] == 0xA5);
}
static void test_fold() {
  EXPECT(r1cs_batch_chunks(0) == 0 && r1cs_batch_chunks(65535) == 1 && r1cs_batch_chunks(65536) == 2 && r1cs_batch_chunks(65537) == 2);
  simulate(300, 6, 300);
  simulate(300, 6, 317);
  simulate(65, 3, 70);
  simulate(1, 3, 1);
  simulate(3, 65537, 5);                                   // chunks of 65535 and 2
  size_t clean = 0, dirty = 0;
  for (size_t b = 0; b < 6; ++b) {
    bool any = false;
    for (size_t row = 0; row < 300; ++row) any = any || row_is_bad(b, row);
    ++(any ? dirty : clean);
  }
  EXPECT(clean >= 1 && dirty >= 2);                        // the simulated batch has both kinds
  if (!failures) std::printf("ok: fold\n");
}

int main() {
  test_args();
  u_cases<Fr, HostFrP>("Fr");
  u_cases<Fq, HostFqP>("Fq");
#ifndef KG_R1CS_HOST_PLAIN_ONLY
  u_cases<FrC, HostFrP>("Fr checked");
  u_cases<FqC, HostFqP>("Fq checked");
#endif
  test_split();
  test_fold();
  if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
  std::printf("ok: r1cs check batch host\n");
  return 0;
}
