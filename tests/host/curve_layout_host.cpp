// curve_layout_host.cpp -- kogarashi_amd/csrc/curve_layout.h as a stand-alone program (tests/test_curve_layout_host.py builds it with g++,
// plain and with -fsanitize=address,undefined, and runs it): the curve ids that are accepted, and every layout function of the three
// curves against the literal sizes of the ABI and of the kernels' scratch forms.
// Prints "<checks> checks, <failures> failures"; the exit status is 0 only without failures.
#include <cstdio>
#include "../../kogarashi_amd/csrc/curve_layout.h"

using namespace kg;

static long g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// the functions are constexpr: a size is usable where a constant is needed
static_assert(coord_words64(KG_G2) == 8 && xyzz_words64(KG_G1) == 16, "curve_layout.h in a constant expression");

int main() {
  CHECK(KG_G1 == 0 && KG_GRUMPKIN == 1 && KG_G2 == 2);
  const bool ok[5] = {false, true, true, true, false};
  for (int curve = -1; curve <= 3; ++curve) CHECK(curve_ok(curve) == ok[curve + 1]);
  CHECK(!curve_ok(1 << 30) && !curve_ok(-(1 << 30)));

  struct Want { int curve; size_t coord, affine, projective, xyzz, res64, res29, raw; int field; };
  const Want want[3] = {{KG_G1, 4, 8, 12, 16, 16, 18, 36, KG_FR},
                        {KG_GRUMPKIN, 4, 8, 12, 16, 16, 18, 36, KG_FQ},
                        {KG_G2, 8, 16, 24, 32, 32, 36, 72, KG_FR}};
  for (const Want& w : want) {
    CHECK(coord_words64(w.curve) == w.coord);
    CHECK(affine_words64(w.curve) == w.affine);
    CHECK(projective_words64(w.curve) == w.projective);
    CHECK(xyzz_words64(w.curve) == w.xyzz);
    CHECK(resident_words32(w.curve, true) == w.res64);
    CHECK(resident_words32(w.curve, false) == w.res29);
    CHECK(raw_xyzz_words32(w.curve) == w.raw);
    CHECK(scalar_field(w.curve) == w.field);
  }
  // the byte counts the callers derive: an ABI base, a resident base in either form
  CHECK(affine_words64(KG_G1) * 8 == 64 && affine_words64(KG_G2) * 8 == 128);
  CHECK(resident_words32(KG_G1, true) * 4 == 64 && resident_words32(KG_G2, true) * 4 == 128);
  CHECK(resident_words32(KG_G1, false) * 4 == 72 && resident_words32(KG_G2, false) * 4 == 144);
  std::printf("%ld checks, %ld failures\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
