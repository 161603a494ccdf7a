// r1cs_check_host.cpp -- the row arithmetic of kg_r1cs_check (kogarashi_amd/csrc/vecops.h: dot_step / dot_merge row sums, sat_residual_row,
// is_zero_mod_p -- the lines vec.hip's kernels are built from) compiled for the host with g++, as a stand-alone program:
// tests/test_r1cs_check_host.py writes a case file, runs this and compares every status byte with what Python integers give.  The same source
// is built a second time with -fsanitize=address,undefined.
//
//   r1cs_check_host <cases.bin> <status.bin> [checked]
//
// cases.bin: records until the end of the file (tests/r1cs_cases.py: write_record), each  u32 field (0 Fr, 1 Fq) | u32 flags (1: u given,
// 2: E given) | u64 m | u64 nvars | for A, B, C: u64 nnz, row_ptr (m + 1 u64), col (nnz u64), val (4 nnz u64) | z (4 nvars u64) | u (4 u64,
// when given) | E (4 m u64, when given).  status.bin: the m status bytes of every record, in order.  Rows are summed as the kernels sum them:
// up to 48 entries in every matrix by one accumulator, longer ones by 64 strided accumulators merged as the shuffle tree merges them.
// "checked" runs the same templates on the bound-tracking FpChecked type (it aborts when a column, limb or value bound of fp29.h could be
// exceeded) -- same bytes expected.  -DKG_R1CS_HOST_PLAIN_ONLY leaves that mode out (the sanitizer build).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/vecops.h"
#include "../../kogarashi_amd/csrc/host_fp.h"
#include "../../kogarashi_amd/csrc/r1cs_batch.h"      // SHORT_ROW

using namespace kg;

template <class F> struct RawIn;
template <class P> struct RawIn<Fp<P>> { static Fp<P> in(const uint32_t* w) { return limbs_from_words<P>(w); } };
#ifndef KG_R1CS_HOST_PLAIN_ONLY
#include "../../kogarashi_amd/csrc/fp29_checked.h"
template <class P> struct RawIn<FpChecked<P>> { static FpChecked<P> in(const uint32_t* w) { return FpChecked<P>::wrap(limbs_from_words<P>(w), 5.4); } };   // any 256-bit input
#endif


struct Csr { std::vector<uint64_t> rp, col, val; };

template <class F>
static F row_sum(const Csr& a, size_t row, const uint64_t* z, int lanes) {
  std::vector<F> part(lanes, F::zero());
  for (uint64_t e = a.rp[row]; e < a.rp[row + 1]; ++e) {
    uint32_t wv[8], wz[8];
    std::memcpy(wv, &a.val[4 * e], 32);
    std::memcpy(wz, z + 4 * a.col[e], 32);
    F& s = part[(e - a.rp[row]) % lanes];
    s = dot_step(s, RawIn<F>::in(wz), RawIn<F>::in(wv));
  }
  for (int d = lanes / 2; d >= 1; d >>= 1)            // lane i ends with what lanes i and i ^ d held: lane 0's value is the tree's
    for (int i = 0; i < d; ++i) part[i] = dot_merge(part[i], part[i + d]);
  return part[0];
}

template <class F, class HostP>
static void run(const Csr (&mat)[3], size_t m, const uint64_t* z, const uint64_t* u, const uint64_t* e, uint8_t* st) {
  using P = typename F::Params;
  uint32_t wu[8];
  std::memcpy(wu, u ? u : HostP::ONE, 32);            // no u: the field's Montgomery one
  const F us = mul(RawIn<F>::in(wu), F::from_const(P::C_XT_U));        // u * 2^266 (the kernel gets it from ten host-side doublings)
  for (size_t i = 0; i < m; ++i) {
    bool is_long = false;
    for (const Csr& a : mat) is_long = is_long || a.rp[i + 1] - a.rp[i] > SHORT_ROW;
    const int lanes = is_long ? 64 : 1;
    const F az = row_sum<F>(mat[0], i, z, lanes), bz = row_sum<F>(mat[1], i, z, lanes), cz = row_sum<F>(mat[2], i, z, lanes);
    F er = F::zero();
    if (e) {
      uint32_t we[8];
      std::memcpy(we, e + 4 * i, 32);
      er = RawIn<F>::in(we);
    }
    st[i] = is_zero_mod_p(sat_residual_row(az, bz, cz, us, er, F::from_const(P::C_XT_HAD))) ? 0 : 1;
  }
}

static bool read_words(std::FILE* in, std::vector<uint64_t>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 8, n, in) == n;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s cases.bin status.bin [checked]\n", argv[0]); return 2; }
  const bool checked = argc > 3 && std::strcmp(argv[3], "checked") == 0;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
  for (;;) {
    uint32_t head[2];
    uint64_t dims[2];
    if (std::fread(head, 4, 2, in) != 2) break;
    if (std::fread(dims, 8, 2, in) != 2 || head[0] > 1 || (head[1] & ~3u) || dims[0] > (1u << 24) || dims[1] > (1u << 24)) { std::fprintf(stderr, "bad record\n"); return 3; }
    const size_t m = dims[0], nvars = dims[1];
    Csr mat[3];
    for (Csr& a : mat) {
      uint64_t nnz;
      if (std::fread(&nnz, 8, 1, in) != 1 || nnz > (1u << 26) || !read_words(in, a.rp, m + 1) || !read_words(in, a.col, nnz) || !read_words(in, a.val, 4 * nnz)) {
        std::fprintf(stderr, "short record\n");
        return 3;
      }
      bool ok = a.rp[0] == 0 && a.rp[m] == nnz;         // the entry trusts its matrices; this program checks what it was handed
      for (size_t i = 0; i < m; ++i) ok = ok && a.rp[i] <= a.rp[i + 1];
      for (uint64_t c : a.col) ok = ok && c < nvars;
      if (!ok) { std::fprintf(stderr, "malformed matrix\n"); return 3; }
    }
    std::vector<uint64_t> z, u, e;
    if (!read_words(in, z, 4 * nvars) || !read_words(in, u, (head[1] & 1) ? 4 : 0) || !read_words(in, e, (head[1] & 2) ? 4 * m : 0)) { std::fprintf(stderr, "short record\n"); return 3; }
    const uint64_t* pu = (head[1] & 1) ? u.data() : nullptr;
    const uint64_t* pe = (head[1] & 2) ? e.data() : nullptr;
    std::vector<uint8_t> st(m);
#ifndef KG_R1CS_HOST_PLAIN_ONLY
    if (checked) {
      if (head[0] == 0) run<FrC, HostFrP>(mat, m, z.data(), pu, pe, st.data());
      else run<FqC, HostFqP>(mat, m, z.data(), pu, pe, st.data());
    } else
#else
    if (checked) { std::fprintf(stderr, "built without the checked mode\n"); return 2; }
#endif
    if (head[0] == 0) run<Fr, HostFrP>(mat, m, z.data(), pu, pe, st.data());
    else run<Fq, HostFqP>(mat, m, z.data(), pu, pe, st.data());
    if (m && std::fwrite(st.data(), 1, m, out) != m) return 4;
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 4;
}
