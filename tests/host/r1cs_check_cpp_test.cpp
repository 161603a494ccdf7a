// r1cs_check_cpp_test.cpp -- R1csShape::is_sat and is_sat_relaxed of include/kogarashi_amd.hpp from a C++ host that links libkogarashi_amd.so
// only.  tests/test_gpu_r1cs_check.py writes one case, runs this on the GPU and compares what it prints with the statuses Python integers give.
//
//   r1cs_check_cpp_test <case.bin>
//
// case.bin: one record of tests/r1cs_cases.py write_record with u and E given (flags = 3): u32 field | u32 flags | u64 m | u64 nvars | for A, B,
// C: u64 nnz, row_ptr, col, val | z | u | E.
#include <cstdio>
#include <vector>
#include "../../include/kogarashi_amd.hpp"

using namespace kogarashi;

static bool words(std::FILE* f, std::vector<uint64_t>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), 8, n, f) == n; }
static bool elems(std::FILE* f, std::vector<Fe>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), 32, n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[2];
  uint64_t dims[2];
  if (std::fread(head, 4, 2, f) != 2 || std::fread(dims, 8, 2, f) != 2 || head[0] > 1 || head[1] != 3 || dims[0] > 4096 || dims[1] > 4096) return 3;
  const size_t m = dims[0], nvars = dims[1];
  SparseMatrix mat[3];
  for (SparseMatrix& a : mat) {
    uint64_t nnz;
    if (std::fread(&nnz, 8, 1, f) != 1 || nnz > (1u << 20) || !words(f, a.row_ptr, m + 1) || !words(f, a.col, nnz) || !elems(f, a.val, nnz)) return 3;
  }
  std::vector<Fe> z, u, e;
  if (!elems(f, z, nvars) || !elems(f, u, 1) || !elems(f, e, m)) return 3;
  std::fclose(f);
  try {
    Context c(0);
    R1csShape shape(c, mat[0], mat[1], mat[2], head[0] == 0 ? KG_FR : KG_FQ);
    std::vector<uint8_t> st;
    R1csShape::Sat r = shape.is_sat_relaxed(z, u[0], e, &st);
    std::printf("relaxed: sat %d bad %zu first %zu status", r ? 1 : 0, r.bad, r.first_bad);
    for (uint8_t s : st) std::printf(" %d", (int)s);
    r = shape.is_sat(z, &st);
    std::printf("\nplain: sat %d bad %zu first %zu status", r ? 1 : 0, r.bad, r.first_bad);
    for (uint8_t s : st) std::printf(" %d", (int)s);
    r = shape.is_sat(z);
    std::printf("\nplain, no status: bad %zu first %zu", r.bad, r.first_bad);
    std::printf("\nok: r1cs check wrappers\n");
  } catch (const std::exception& ex) {
    std::printf("\nFAILED: %s\n", ex.what());
    return 1;
  }
  return 0;
}
