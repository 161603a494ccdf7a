// r1cs_batch_host.cpp -- the parts of the batched CSR product (kg_r1cs_prod_batch) and of the batched prover's R1CS form
// (kg_groth16_prove_r1cs_batch) that need no device, as a stand-alone program over kogarashi_amd/csrc/r1cs_batch.h alone
// (tests/test_r1cs_batch_host.py builds it with g++, plain and with -fsanitize=address,undefined, and runs it): the chunk rule, the grid
// rule of the list launches and both argument checks.
// Prints "<checks> checks, <failures> failures"; the exit status is 0 only without failures.
#include <cstdio>
#include <vector>
#include "../../kogarashi_amd/csrc/r1cs_batch.h"

using namespace kg;

static long g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

struct Csr { const void* d_row_ptr; const void* d_col; const void* d_val; };

static void chunk_rule() {
  CHECK(R1CS_BATCH_GRID_Y_MAX == 65535);
  const size_t counts[] = {0, 1, 2, 65534, 65535, 65536, 65537, 2 * 65535, 2 * 65535 + 1, (size_t)1 << 20};
  const size_t want_chunks[] = {0, 1, 1, 1, 1, 2, 2, 2, 3, 17};
  for (int k = 0; k < 10; ++k) {
    const size_t count = counts[k], chunks = r1cs_batch_chunks(count);
    CHECK(chunks == want_chunks[k]);
    std::vector<unsigned char> seen(count, 0);                       // every vector exactly once, in order, no chunk empty or too long
    size_t next = 0;
    bool once = true;
    for (size_t i = 0; i < chunks; ++i) {
      const R1csBatchChunk ch = r1cs_batch_chunk(count, i);
      CHECK(ch.first == next && ch.count >= 1 && ch.count <= R1CS_BATCH_GRID_Y_MAX && ch.first + ch.count <= count);
      for (size_t b = ch.first; b < ch.first + ch.count && b < count; ++b) once = once && seen[b]++ == 0;
      next = ch.first + ch.count;
    }
    CHECK(next == count && once);
    for (size_t b = 0; b < count; ++b) once = once && seen[b] == 1;
    CHECK(once);
  }
  CHECK(r1cs_batch_chunk(65537, 1).first == 65535 && r1cs_batch_chunk(65537, 1).count == 2);
  CHECK(r1cs_batch_chunks(SIZE_MAX) == SIZE_MAX / 65535 + (SIZE_MAX % 65535 ? 1 : 0));
  // the list launches' x dimension: the single product's blocks spread over the vectors, never zero, never more than the single product's
  CHECK(r1cs_batch_grid_x(256, 1) == 256 && r1cs_batch_grid_x(256, 2) == 128 && r1cs_batch_grid_x(256, 3) == 85 && r1cs_batch_grid_x(256, 256) == 1);
  CHECK(r1cs_batch_grid_x(256, 257) == 1 && r1cs_batch_grid_x(256, 65535) == 1 && r1cs_batch_grid_x(64, 5) == 12 && r1cs_batch_grid_x(64, 65) == 1);
  CHECK(r1cs_batch_grid_x(64, 0) == 64);
}

static void prod_args() {
  int x = 0;
  const void* p = &x;                                                // never dereferenced
  CHECK(r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 155, 5, p, 300) && r1cs_batch_args_ok(p, 1, p, p, p, 300, p, 158, 5, p, 305));
  CHECK(r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 0, 5, p, 300));                                    // one vector read five times
  CHECK(!r1cs_batch_args_ok(nullptr, 0, p, p, p, 300, p, 155, 5, p, 300));                           // a null ctx
  CHECK(!r1cs_batch_args_ok(p, 2, p, p, p, 300, p, 155, 5, p, 300) && !r1cs_batch_args_ok(p, -1, p, p, p, 300, p, 155, 5, p, 300));
  for (int null_at = 0; null_at < 5; ++null_at) {                                                    // every array, one at a time
    const void* a[5] = {p, p, p, p, p};
    a[null_at] = nullptr;
    CHECK(!r1cs_batch_args_ok(p, 0, a[0], a[1], a[2], 300, a[3], 155, 5, a[4], 300));
    CHECK(r1cs_batch_args_ok(p, 0, a[0], a[1], a[2], 300, a[3], 155, 0, a[4], 300));                 // count == 0: nothing is read or written
    CHECK(r1cs_batch_args_ok(p, 0, a[0], a[1], a[2], 0, a[3], 155, 5, a[4], 0));                     // m == 0 likewise
  }
  CHECK(r1cs_batch_empty(0, 5) && r1cs_batch_empty(300, 0) && r1cs_batch_empty(0, 0) && !r1cs_batch_empty(1, 1));
  CHECK(!r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 155, 5, p, 299) && !r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 155, 0, p, 299));      // out_stride < m
  CHECK(!r1cs_batch_args_ok(nullptr, 0, p, p, p, 300, p, 155, 0, p, 300) && !r1cs_batch_args_ok(p, 7, p, p, p, 0, p, 155, 5, p, 0));    // ... also when empty
  const size_t two32 = (size_t)1 << 32;
  CHECK(r1cs_batch_args_ok(p, 0, p, p, p, two32 - 1, p, 1, 1, p, two32 - 1));
  CHECK(!r1cs_batch_args_ok(p, 0, p, p, p, two32, p, 1, 1, p, two32) && !r1cs_batch_args_ok(p, 0, p, p, p, two32, p, 1, 0, p, two32));
  // count * stride * 32 beyond size_t
  CHECK(!r1cs_batch_args_ok(p, 0, p, p, p, 300, p, (size_t)1 << 60, 16, p, 300) && !r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 155, 16, p, (size_t)1 << 60));
  CHECK(r1cs_batch_args_ok(p, 0, p, p, p, 300, p, SIZE_MAX / 64, 2, p, SIZE_MAX / 64));
  CHECK(!r1cs_batch_args_ok(p, 0, p, p, p, 300, p, SIZE_MAX / 64 + 1, 2, p, 300) && !r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 155, 2, p, SIZE_MAX / 64 + 1));
  CHECK(!r1cs_batch_args_ok(p, 0, p, p, p, 300, p, SIZE_MAX, 2, p, 300) && !r1cs_batch_args_ok(p, 0, p, p, p, 300, p, 155, SIZE_MAX, p, 300));
  CHECK(r1cs_batch_args_ok(p, 0, p, p, p, 1, p, 0, SIZE_MAX / 32, p, 1) && !r1cs_batch_args_ok(p, 0, p, p, p, 1, p, 0, SIZE_MAX / 32 + 1, p, 1));
}

static void prover_args() {
  int x = 0;
  const void* p = &x;
  const Csr full{p, p, p};
  auto ok = [&](const void* ctx, const void* crs, size_t m, size_t l, size_t w, const Csr* a, const Csr* b, const Csr* c, const void* dx, size_t xs, const void* dw,
                size_t ws, const void* r, const void* s, size_t count, const void* out, const void* inf) {
    return g16_r1cs_batch_args_ok<Csr>(ctx, crs, m, l, w, a, b, c, dx, xs, dw, ws, r, s, count, out, inf);
  };
  CHECK(ok(p, p, 5, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p) && ok(p, p, 5, 2, 5, &full, &full, &full, p, 4, p, 11, p, p, 3, p, p));
  CHECK(!ok(nullptr, p, 5, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p) && !ok(p, nullptr, 5, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p));
  for (int which = 0; which < 3; ++which) {                                                          // a null kg_csr, a null member array
    const Csr* m3[3] = {&full, &full, &full};
    m3[which] = nullptr;
    CHECK(!ok(p, p, 5, 2, 5, m3[0], m3[1], m3[2], p, 2, p, 5, p, p, 3, p, p));
    CHECK(ok(p, p, 5, 2, 5, m3[0], m3[1], m3[2], p, 2, p, 5, p, p, 0, p, p));                        // count == 0: never looked at
    for (int member = 0; member < 3; ++member) {
      Csr part = full;
      (member == 0 ? part.d_row_ptr : (member == 1 ? part.d_col : part.d_val)) = nullptr;
      m3[which] = &part;
      CHECK(!ok(p, p, 5, 2, 5, m3[0], m3[1], m3[2], p, 2, p, 5, p, p, 3, p, p));
      CHECK(ok(p, p, 5, 2, 5, m3[0], m3[1], m3[2], p, 2, p, 5, p, p, 0, p, p));
    }
  }
  for (int null_at = 0; null_at < 6; ++null_at) {                                                    // x, w, r, s, proofs, flags
    const void* a[6] = {p, p, p, p, p, p};
    a[null_at] = nullptr;
    CHECK(!ok(p, p, 5, 2, 5, &full, &full, &full, a[0], 2, a[1], 5, a[2], a[3], 3, a[4], a[5]));
    CHECK(ok(p, p, 5, 2, 5, &full, &full, &full, a[0], 2, a[1], 5, a[2], a[3], 0, a[4], a[5]));
  }
  CHECK(ok(p, p, 5, 7, 0, &full, &full, &full, p, 7, nullptr, 0, p, p, 3, p, p));                    // no witness values: w may be null
  CHECK(!ok(p, p, 5, 2, 5, &full, &full, &full, p, 1, p, 5, p, p, 3, p, p) && !ok(p, p, 5, 2, 5, &full, &full, &full, p, 2, p, 4, p, p, 3, p, p));      // a short stride
  CHECK(!ok(p, p, 5, 2, 5, &full, &full, &full, p, 1, p, 5, p, p, 0, p, p));                         // ... also for an empty batch
  CHECK(!ok(p, p, 0, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p) && !ok(p, p, 5, 0, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p));
  CHECK(!ok(p, p, ((size_t)1 << 28) + 1, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p) && ok(p, p, (size_t)1 << 28, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, 3, p, p));
  CHECK(!ok(p, p, 5, 2, 5, &full, &full, &full, p, SIZE_MAX / 64 + 1, p, 5, p, p, 2, p, p) && ok(p, p, 5, 2, 5, &full, &full, &full, p, SIZE_MAX / 64, p, 5, p, p, 2, p, p));
  CHECK(!ok(p, p, 5, 2, 5, &full, &full, &full, p, 2, p, SIZE_MAX, p, p, 2, p, p));
  CHECK(!ok(p, p, 5, 2, 5, &full, &full, &full, p, 2, p, 5, p, p, SIZE_MAX / 256 + 1, p, p));        // count proofs of 256 bytes
  CHECK(!ok(p, p, 5, 2, SIZE_MAX / 64 + 1, &full, &full, &full, p, 2, p, SIZE_MAX / 64 + 1, p, p, 1, p, p));       // (l + m_l_1) * 32
}

int main() {
  chunk_rule();
  prod_args();
  prover_args();
  std::printf("%ld checks, %ld failures\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
