// ntt_batch_plan_host.cpp -- the pure parts of the batched transform (kogarashi_amd/csrc/ntt_batch.h) without HIP and without a device:
// the group rule, the group boundaries, the per-step strides and the argument checks.  A stand-alone program (tests/test_ntt_batch_host.py
// builds it plain and with -fsanitize=address,undefined); prints one line per failed check and returns the number of failures.
#include <cstdio>
#include <vector>
#include "../../kogarashi_amd/csrc/ntt_batch.h"

using namespace kg;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++failures;                                         \
      std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
    }                                                     \
  } while (0)

// the rule as the header's documentation states it, written out independently
static size_t want_per_launch(uint32_t log_n) {
  if (log_n <= 11) return 65535;
  const size_t s = ((size_t)1 << 23) >> log_n;
  return s ? s : 1;
}

int main() {
  CHECK(NTT_BATCH_GRID_Y_MAX == 65535 && NTT_BATCH_SCRATCH_LOG == 23, "the two constants");
  CHECK(want_per_launch(12) == 2048 && want_per_launch(22) == 2 && want_per_launch(23) == 1 && want_per_launch(28) == 1, "the rule's own examples");
  for (uint32_t log_n = 1; log_n <= 28; ++log_n) {
    const size_t n = (size_t)1 << log_n, per = ntt_batch_per_launch(log_n);
    CHECK(per == want_per_launch(log_n), "log_n %u: per_launch %zu", log_n, per);
    CHECK(per >= 1 && per <= 65535, "log_n %u: per_launch %zu", log_n, per);
    const size_t counts[] = {1, 2, per - 1, per, per + 1, 2 * per + 1, 70000};
    for (size_t count : counts) {
      const size_t groups = ntt_batch_groups(log_n, count);
      if (count == 0) {                                   // per == 1: per - 1
        CHECK(groups == 0, "log_n %u: an empty batch has %zu groups", log_n, groups);
        CHECK(ntt_batch_scratch_elems(log_n, count) == 0, "log_n %u: an empty batch needs scratch", log_n);
        continue;
      }
      CHECK(groups == (count + per - 1) / per, "log_n %u count %zu: %zu groups", log_n, count, groups);
      size_t next = 0;
      for (size_t g = 0; g < groups; ++g) {
        const NttBatchGroup grp = ntt_batch_group(per, count, g);
        CHECK(grp.first == next, "log_n %u count %zu group %zu: begins at %zu, the one before ended at %zu", log_n, count, g, grp.first, next);
        CHECK(grp.count >= 1 && grp.count <= 65535, "log_n %u count %zu group %zu: %zu transforms", log_n, count, g, grp.count);
        if (log_n > 11) CHECK(grp.count * n <= ((size_t)1 << 23) || grp.count == 1, "log_n %u count %zu group %zu: scratch of %zu elements", log_n, count, g, grp.count * n);
        CHECK(g + 1 == groups || grp.count == per, "log_n %u count %zu group %zu: a group before the last is not full", log_n, count, g);
        next = grp.first + grp.count;
      }
      CHECK(next == count, "log_n %u count %zu: the groups end at %zu", log_n, count, next);
      const size_t scratch = ntt_batch_scratch_elems(log_n, count);
      if (log_n <= 11) CHECK(scratch == 0, "log_n %u: a one-step plan asks for scratch", log_n);
      else {
        CHECK(scratch == (count < per ? count : per) * n, "log_n %u count %zu: scratch %zu", log_n, count, scratch);
        CHECK(scratch <= ((size_t)1 << 23) || per == 1, "log_n %u count %zu: scratch %zu", log_n, count, scratch);
      }
    }
  }
  CHECK(ntt_batch_per_launch(0) == 0 && ntt_batch_per_launch(29) == 0 && ntt_batch_groups(0, 5) == 0 && ntt_batch_groups(29, 5) == 0, "sizes outside 1..28");
  CHECK(ntt_batch_groups(10, 0) == 0, "an empty batch");

  // strides per plan step: single (stride, stride); A (stride, n); B (n, n); C (n, stride)
  const size_t n = 4096, stride = 4099;
  auto eq = [](NttBatchStrides s, size_t in, size_t out) { return s.in == in && s.out == out; };
  CHECK(eq(ntt_batch_step_strides(1, 0, n, stride), stride, stride), "single step");
  CHECK(eq(ntt_batch_step_strides(2, 0, n, stride), stride, n), "two steps, A");
  CHECK(eq(ntt_batch_step_strides(2, 1, n, stride), n, stride), "two steps, C");
  CHECK(eq(ntt_batch_step_strides(3, 0, n, stride), stride, n), "three steps, A");
  CHECK(eq(ntt_batch_step_strides(3, 1, n, stride), n, n), "three steps, B");
  CHECK(eq(ntt_batch_step_strides(3, 2, n, stride), n, stride), "three steps, C");

  // argument checks
  int ctx = 0, data = 0;
  CHECK(ntt_batch_args_ok(&ctx, &data, 12, 3, 4096) && ntt_batch_args_ok(&ctx, &data, 12, 3, 5000) && ntt_batch_args_ok(&ctx, &data, 1, 0, 2), "acceptable");
  CHECK(!ntt_batch_args_ok(nullptr, &data, 12, 3, 4096) && !ntt_batch_args_ok(&ctx, nullptr, 12, 3, 4096), "null pointers");
  CHECK(!ntt_batch_args_ok(&ctx, &data, 12, 3, 4095) && !ntt_batch_args_ok(&ctx, &data, 1, 1, 1) && !ntt_batch_args_ok(&ctx, &data, 28, 1, ((size_t)1 << 28) - 1), "stride < n");
  CHECK(!ntt_batch_args_ok(&ctx, &data, 0, 1, 4096) && !ntt_batch_args_ok(&ctx, &data, 29, 1, (size_t)1 << 29), "log_n 0 and 29");
  const size_t top = SIZE_MAX / 32;                      // the most elements whose bytes fit a size_t
  CHECK(ntt_batch_args_ok(&ctx, &data, 4, top / 16, 16), "count * stride * 32 just fits");
  CHECK(!ntt_batch_args_ok(&ctx, &data, 4, top / 16 + 1, 16), "count * stride * 32 overflows by one transform");
  CHECK(!ntt_batch_args_ok(&ctx, &data, 4, SIZE_MAX, 16) && !ntt_batch_args_ok(&ctx, &data, 4, 2, SIZE_MAX) && !ntt_batch_args_ok(&ctx, &data, 4, 3, SIZE_MAX / 2), "byte overflow");
  CHECK(ntt_batch_args_ok(&ctx, &data, 4, 1, top) && !ntt_batch_args_ok(&ctx, &data, 4, 1, top + 1), "one transform, the stride alone overflows");

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
