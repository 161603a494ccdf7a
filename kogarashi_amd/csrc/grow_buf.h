// grow_buf.h -- GrowBuf<Mem>: a buffer that owns its memory and only ever grows.  No HIP in here: the memory comes from the policy Mem
// (common.h has the device and the pinned one), so a plain host program can test the rule (tests/host/grow_buf_test.cpp).
//
// Mem is a small copyable value with
//   int  alloc(void** p, size_t bytes)      0 and *p on success; anything else is a status that ensure() hands back as it is
//   void release(void* p)
//   static constexpr bool drains            true: release waits for whatever may still use the memory --
//   void drain_before_release()             called before every release (needed only when drains is true)
// The buffer keeps the policy that made its allocation and releases through it.
#pragma once
#include <cstddef>
#include <utility>

namespace kg {

template <class Mem>
class GrowBuf {
 public:
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  GrowBuf(GrowBuf&& o) noexcept : mem_(o.mem_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  GrowBuf& operator=(GrowBuf&& o) noexcept {
    if (this != &o) { reset(); mem_ = o.mem_; p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~GrowBuf() { reset(); }

  // THE grow-only rule: a request that fits changes nothing; otherwise the old block goes (drained first) and a block of bytes + slack
  // takes its place.  When the allocation is refused the buffer is left empty, so a later, smaller request starts afresh.
  int ensure(const Mem& mem, size_t bytes, size_t slack = 0) {
    if (bytes <= cap_) return 0;
    reset();
    mem_ = mem;
    const int rc = mem_.alloc(&p_, bytes + slack);
    if (rc != 0) { p_ = nullptr; return rc; }
    cap_ = bytes + slack;
    return 0;
  }
  void reset() {
    if (!p_) return;
    if constexpr (Mem::drains) mem_.drain_before_release();
    mem_.release(p_);
    p_ = nullptr; cap_ = 0;
  }
  void* get() const { return p_; }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }
  const Mem& mem() const { return mem_; }

 private:
  Mem mem_{};
  void* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace kg
