// points_check_cpp_test.cpp -- one call to each point-validation wrapper of include/kogarashi_amd.hpp (check_points, Prover::check_crs) from a
// C++ host that links libkogarashi_amd.so only.  tests/test_gpu_points_check.py writes the points, runs this on the GPU and compares what it
// prints with the statuses Python integers give.
//
//   points_check_cpp_test <points.bin>
//
// points.bin: u64 n1 | u64 n2 | n1 G1 points (8 words) | n2 G2 points (16 words); n1 >= 9, n2 >= 4.  A circuit with l = 1, m_l_1 = 1, m = 2
// takes its Parameters from them: h = G1[0..1), l = G1[1..2), a = G1[2..4), b_g1 = G1[4..6), alpha / beta / delta = G1[6..9), b_g2 = G2[0..2),
// beta_g2 = G2[2], delta_g2 = G2[3].
#include <cstdio>
#include <vector>
#include "../../include/kogarashi_amd.hpp"

using namespace kogarashi;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n[2];
  if (std::fread(n, 8, 2, f) != 2 || n[0] < 9 || n[1] < 4 || n[0] > 4096 || n[1] > 4096) return 3;
  std::vector<uint64_t> w1(8 * n[0]), w2(16 * n[1]);
  if (std::fread(w1.data(), 8, w1.size(), f) != w1.size() || std::fread(w2.data(), 8, w2.size(), f) != w2.size()) return 3;
  std::fclose(f);
  std::vector<G1Affine> g1;
  std::vector<G2Affine> g2;
  for (size_t i = 0; i < n[0]; ++i) g1.push_back(detail::g1_from(&w1[8 * i], false));
  for (size_t i = 0; i < n[1]; ++i) g2.push_back(detail::g2_from(&w2[16 * i], false));
  try {
    Context c(0);
    std::vector<uint8_t> st;
    PointsCheck r = check_points(c, g1, KG_G1, true, &st);
    std::printf("g1: bad %zu first %zu status", r.bad, r.first_bad);
    for (uint8_t s : st) std::printf(" %d", (int)s);
    r = check_points(c, g2, KG_G2, true, &st);
    std::printf("\ng2: bad %zu first %zu status", r.bad, r.first_bad);
    for (uint8_t s : st) std::printf(" %d", (int)s);
    r = check_points(c, g2, KG_G2, false, &st);
    std::printf("\ng2 curve only: bad %zu first %zu status", r.bad, r.first_bad);
    for (uint8_t s : st) std::printf(" %d", (int)s);
    Parameters p;
    p.h.assign(g1.begin(), g1.begin() + 1);
    p.l.assign(g1.begin() + 1, g1.begin() + 2);
    p.a.assign(g1.begin() + 2, g1.begin() + 4);
    p.b_g1.assign(g1.begin() + 4, g1.begin() + 6);
    p.alpha_g1 = g1[6]; p.beta_g1 = g1[7]; p.delta_g1 = g1[8];
    p.b_g2.assign(g2.begin(), g2.begin() + 2);
    p.beta_g2 = g2[2]; p.delta_g2 = g2[3];
    Prover prover(c, p, 2, 1, 1);
    std::printf("\ncrs:");
    for (size_t v : prover.check_crs()) std::printf(" %zu", v);
    std::printf("\nok: points check wrappers\n");
  } catch (const std::exception& e) {
    std::printf("\nFAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
