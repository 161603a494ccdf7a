// ntt_batch_cpp_test.cpp -- Fft::batch and Fft::divide_by_z_on_coset_batch of include/kogarashi_amd.hpp against the oracle's C restatement
// of fft.rs, on the GPU box: ragged rows (zero padded per row like prepare_fft), all four transforms and the division, a one-step and a
// two-step size, an empty batch.  Test infrastructure: built and run by tests/test_gpu_ntt_batch_cpp.py; links libkogarashi_amd.so and
// liboracle.so.
#include <cstdio>
#include "../../include/kogarashi_amd.hpp"

typedef uint64_t u64;
extern "C" {
void kgo_gen_scalars(int fd, u64 seed, size_t start, size_t n, u64* out);
struct kgo_fft;
kgo_fft* kgo_fft_new(int k);
void kgo_fft_free(kgo_fft* f);
void kgo_fft_dft(const kgo_fft* f, u64* data, int threads);
void kgo_fft_idft(const kgo_fft* f, u64* data, int threads);
void kgo_fft_coset_dft(const kgo_fft* f, u64* data, int threads);
void kgo_fft_coset_idft(const kgo_fft* f, u64* data, int threads);
void kgo_fft_divide_by_z_on_coset(const kgo_fft* f, u64* data);
}

using namespace kogarashi;
static const u64 SEED = 0x4B6F676172617368ull;
static int failures = 0;
#define CHECK(cond, what)                                                 \
  do {                                                                    \
    if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } \
  } while (0)

static void test_batch(const Context& ctx, int k) {
  const size_t n = (size_t)1 << k;
  std::vector<std::vector<Fe>> rows;
  for (size_t b = 0; b < 3; ++b) {                                      // lengths n, n - 1, n - 2
    std::vector<Fe> v(n - b);
    kgo_gen_scalars(0, SEED + 40 + 8 * k + b, 0, v.size(), reinterpret_cast<u64*>(v.data()));
    rows.push_back(v);
  }
  auto padded = [&](const std::vector<Fe>& v) { std::vector<Fe> p(n, Fe{0, 0, 0, 0}); std::copy(v.begin(), v.end(), p.begin()); return p; };
  kgo_fft* fo = kgo_fft_new(k);
  Fft f(ctx, k);
  struct { const char* name; int inverse, coset; void (*ref)(const kgo_fft*, u64*, int); } ops[] = {
      {"batch dft", 0, 0, kgo_fft_dft}, {"batch idft", 1, 0, kgo_fft_idft}, {"batch coset_dft", 0, 1, kgo_fft_coset_dft}, {"batch coset_idft", 1, 1, kgo_fft_coset_idft}};
  for (auto& op : ops) {
    const std::vector<std::vector<Fe>> got = f.batch(rows, op.inverse, op.coset);
    CHECK(got.size() == rows.size(), op.name);
    for (size_t b = 0; b < rows.size() && b < got.size(); ++b) {
      std::vector<Fe> want = padded(rows[b]);
      op.ref(fo, reinterpret_cast<u64*>(want.data()), 4);
      CHECK(got[b] == want, op.name);
    }
  }
  const std::vector<std::vector<Fe>> got = f.divide_by_z_on_coset_batch(rows);
  CHECK(got.size() == rows.size(), "divide_by_z_on_coset_batch");
  for (size_t b = 0; b < rows.size() && b < got.size(); ++b) {
    std::vector<Fe> want = padded(rows[b]);
    kgo_fft_divide_by_z_on_coset(fo, reinterpret_cast<u64*>(want.data()));
    CHECK(got[b] == want, "divide_by_z_on_coset_batch");
  }
  CHECK(f.batch({}).empty() && f.divide_by_z_on_coset_batch({}).empty(), "an empty batch");
  kgo_fft_free(fo);
}

int main() {
  try {
    Context ctx(0);
    test_batch(ctx, 6);
    test_batch(ctx, 13);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
  std::printf(failures ? "FAILED: %d checks\n" : "ok: Fft::batch and Fft::divide_by_z_on_coset_batch match the oracle\n", failures);
  return failures ? 1 : 0;
}
