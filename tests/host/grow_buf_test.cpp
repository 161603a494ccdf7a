// grow_buf_test.cpp -- the grow-only owner (kogarashi_amd/csrc/grow_buf.h) on its own, with a memory policy that counts: what a request
// that fits costs, the order drain -> release -> alloc of a growth, the state after a refused allocation, moves, and that every block is
// released exactly once when a buffer, an array of buffers or an erased vector element goes away.  Built with -fsanitize=address,undefined
// by tests/test_grow_buf_host.py (the blocks are real: a double release or a leak is the sanitizer's finding as well as the counters').
#include "../../kogarashi_amd/csrc/grow_buf.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct Log {
  std::string calls;                                        // 'd' drain, 'r' release, 'a' alloc, in order
  int allocs = 0, releases = 0, drains = 0;
  size_t last_bytes = 0, refuse_above = ~(size_t)0;
};
template <bool DRAINS>
struct CountMem {
  Log* log = nullptr;
  static constexpr bool drains = DRAINS;
  int alloc(void** p, size_t bytes) {
    log->calls += 'a'; log->last_bytes = bytes;
    if (bytes > log->refuse_above) { *p = (void*)0x10; return -3; }      // a refusal may leave rubbish in *p
    *p = std::malloc(bytes);
    log->allocs += 1;
    return 0;
  }
  void drain_before_release() { log->calls += 'd'; log->drains += 1; }
  void release(void* p) { log->calls += 'r'; log->releases += 1; std::free(p); }
};
using Mem = CountMem<true>;
using Buf = kg::GrowBuf<Mem>;
struct Holder { int tag; Buf a, b; };                      // the shape of a registered array: two owners in a vector element

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "grow_buf_test: line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
  {                                                         // 1. first request, a request that fits, growth with slack
    Log L;
    Buf b;
    CHECK(!b && b.get() == nullptr && b.capacity() == 0);
    CHECK(b.ensure(Mem{&L}, 0) == 0 && L.calls.empty());    // nothing asked, nothing done
    CHECK(b.ensure(Mem{&L}, 100) == 0 && L.calls == "a" && L.last_bytes == 100 && b.capacity() == 100 && b);
    void* const first = b.get();
    CHECK(b.ensure(Mem{&L}, 100) == 0 && b.ensure(Mem{&L}, 1, 50) == 0 && L.calls == "a" && b.get() == first);      // fits: no call at all
    CHECK(b.ensure(Mem{&L}, 800, 800 / 8) == 0 && L.calls == "adra" && L.last_bytes == 900 && b.capacity() == 900);
    CHECK(b.ensure(Mem{&L}, 900) == 0 && L.calls == "adra");                                                      // the slack is capacity
    CHECK(b.ensure(Mem{&L}, 901) == 0 && L.calls == "adradra" && L.last_bytes == 901);
    b.as<char>()[900] = 1;                                  // the block is as long as it says
    CHECK(L.allocs == 3 && L.releases == 2 && L.drains == 2);
  }
  {                                                         // 2. a refused allocation leaves the buffer empty; a smaller request starts afresh
    Log L;
    L.refuse_above = 1000;
    {
      Buf b;
      CHECK(b.ensure(Mem{&L}, 500) == 0);
      CHECK(b.ensure(Mem{&L}, 2000, 250) == -3 && L.calls == "adra" && L.last_bytes == 2250);      // the policy's status comes back as it is
      CHECK(!b && b.get() == nullptr && b.capacity() == 0);
      CHECK(b.ensure(Mem{&L}, 300) == 0 && L.calls == "adraa" && b.capacity() == 300 && b);        // nothing to drain or release: it was empty
      Buf never;
      CHECK(never.ensure(Mem{&L}, 5000) == -3 && !never);
    }
    CHECK(L.allocs == 2 && L.releases == 2);
  }
  {                                                         // 3. moves leave the source empty and release what the target held
    Log L;
    {
      Buf a, b;
      CHECK(a.ensure(Mem{&L}, 64) == 0 && b.ensure(Mem{&L}, 32) == 0);
      void* const pa = a.get();
      Buf c(std::move(a));
      CHECK(!a && a.capacity() == 0 && c.get() == pa && c.capacity() == 64 && L.releases == 0);
      b = std::move(c);
      CHECK(!c && b.get() == pa && b.capacity() == 64 && L.releases == 1);
      CHECK(a.ensure(Mem{&L}, 8) == 0 && a.capacity() == 8);             // a moved-from buffer is an empty one
      b.reset();
      CHECK(!b && b.capacity() == 0 && L.releases == 2);
      b.reset();
      CHECK(L.releases == 2);
    }
    CHECK(L.allocs == 3 && L.releases == 3 && L.drains == 3);
  }
  {                                                         // 4. arrays, and vector elements that are erased
    Log L;
    {
      Buf arr[5];
      for (int i = 0; i < 5; i += 2) CHECK(arr[i].ensure(Mem{&L}, 16 + i) == 0);
      std::vector<Holder> v;
      for (int i = 0; i < 4; ++i) {
        Holder h{i, {}, {}};
        CHECK(h.a.ensure(Mem{&L}, 40) == 0);
        if (i & 1) CHECK(h.b.ensure(Mem{&L}, 24) == 0);
        v.push_back(std::move(h));
      }
      CHECK(L.allocs == 9 && L.releases == 0);
      void* const keep = v[2].a.get();
      v.erase(v.begin() + 1);                               // element 1 held two blocks
      CHECK(L.releases == 2 && v.size() == 3 && v[1].tag == 2 && v[1].a.get() == keep && v[2].tag == 3 && v[2].b);
    }
    CHECK(L.allocs == 9 && L.releases == 9 && L.drains == 9);
  }
  {                                                         // 5. a policy that opts out of draining
    Log L;
    {
      kg::GrowBuf<CountMem<false>> b;
      CHECK(b.ensure(CountMem<false>{&L}, 10) == 0 && b.ensure(CountMem<false>{&L}, 20) == 0 && L.calls == "ara");
      kg::GrowBuf<CountMem<false>> c(std::move(b));
    }
    CHECK(L.calls == "arar" && L.drains == 0);
  }
  std::printf("grow_buf_test: %d failures\n", failures);
  return failures ? 1 : 0;
}
