// points_check_host.cpp -- the per-point predicates of kg_points_check (kogarashi_amd/csrc/points_check.h: canonical words, curve equation,
// G2 subgroup) compiled for the host with g++, as a stand-alone program: tests/test_points_check_host.py writes a case file, runs this and
// compares every status byte with what Python integers give.  The same source is built a second time with -fsanitize=address,undefined.
//
//   points_check_host <cases.bin> <status.bin> [checked]
//
// cases.bin: records until the end of the file, each  u32 curve (0 G1, 1 Grumpkin, 2 G2) | u32 checks (1 curve, 2 subgroup) | u64 n |
// n * W u64 words (W = 8 or 16: x | y, ABI form) | n flag bytes (non-zero = identity).  status.bin: the n status bytes of every record, in
// order.  "checked" runs the predicates on the bound-tracking FpChecked type instead (it aborts when a column, limb or value bound of
// fp29.h could be exceeded) -- same bytes expected.  -DKG_POINTS_HOST_PLAIN_ONLY leaves that mode out (the sanitizer build: half the code).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kogarashi_amd/csrc/fp29.h"
#include "../../kogarashi_amd/csrc/points_check.h"

using namespace kg;

#ifndef KG_POINTS_HOST_PLAIN_ONLY
#include "../../kogarashi_amd/csrc/fp29_checked.h"
namespace kg { namespace pts {
template <class P> struct Elem<FpChecked<P>> {
  static FpChecked<P> from_ref_words(const uint32_t* w) {
    return mul(FpChecked<P>::wrap(limbs_from_words<P>(w), 5.4), FpChecked<P>::from_const(P::C_FROM_REF));   // any 256-bit input
  }
};
}}
#endif

template <class F>
static void run(const uint64_t* xy, const uint8_t* inf, size_t n, int checks, uint8_t* st) {
  constexpr int W = 2 * pts::Coord<F>::NW;           // u32 words of a point
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[W];
    std::memcpy(w, xy + i * (W / 2), sizeof w);
    st[i] = (checks & 2) ? pts::point_status<F, true>(w, inf[i] != 0) : pts::point_status<F, false>(w, inf[i] != 0);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s cases.bin status.bin [checked]\n", argv[0]); return 2; }
  const bool checked = argc > 3 && std::strcmp(argv[3], "checked") == 0;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
  for (;;) {
    uint32_t head[2];
    uint64_t n;
    if (std::fread(head, 4, 2, in) != 2) break;
    if (std::fread(&n, 8, 1, in) != 1 || head[0] > 2 || (head[1] & ~3u) || head[1] == 0 || n > (1u << 24)) { std::fprintf(stderr, "bad record\n"); return 3; }
    const size_t W = head[0] == 2 ? 16 : 8;
    std::vector<uint64_t> xy(n * W);
    std::vector<uint8_t> inf(n), st(n);
    if ((n && std::fread(xy.data(), 8, n * W, in) != n * W) || (n && std::fread(inf.data(), 1, n, in) != n)) { std::fprintf(stderr, "short record\n"); return 3; }
    const int checks = (int)head[1];
#ifndef KG_POINTS_HOST_PLAIN_ONLY
    if (checked) {
      if (head[0] == 0) run<FqC>(xy.data(), inf.data(), n, checks, st.data());
      else if (head[0] == 1) run<FrC>(xy.data(), inf.data(), n, checks, st.data());
      else run<Fq2C>(xy.data(), inf.data(), n, checks, st.data());
    } else
#else
    if (checked) { std::fprintf(stderr, "built without the checked mode\n"); return 2; }
#endif
    if (head[0] == 0) run<Fq>(xy.data(), inf.data(), n, checks, st.data());
    else if (head[0] == 1) run<Fr>(xy.data(), inf.data(), n, checks, st.data());
    else run<Fq2>(xy.data(), inf.data(), n, checks, st.data());
    if (n && std::fwrite(st.data(), 1, n, out) != n) return 4;
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 4;
}
