// growbuf.hpp — GrowBuf<Mem>: the one owner of a buffer that only grows (the
// device arenas and pinned mirrors every subsystem of the library keeps across
// calls).  Host-only: standard headers alone, no HIP include and no other
// header of the library, so a plain g++ build can test it
// (tools/growbuf_harness.cpp).  Mem supplies the memory:
//   static void* alloc(size_t bytes);  // throws on failure
//   static void free(void* p);         // may throw
// ctx.hpp defines the two policies the library uses (DevBuf, PinnedBuf).
#pragma once
#include <cstddef>
#include <cstring>

namespace gsc {

// sub-buffers of one allocation start on 256-B boundaries
constexpr size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

template <class Mem>
class GrowBuf {
  void* p = nullptr;
  size_t cap = 0;

  // free (a failure is the caller's error), forget, then allocate: a failed
  // allocation leaves an empty buffer, never a dangling pointer
  void regrow(size_t want) {
    if (p) Mem::free(p);
    p = nullptr;
    cap = 0;
    p = Mem::alloc(want);
    cap = want;
  }
  // free and forget; an error from the free is ignored
  void drop() noexcept {
    try {
      if (p) Mem::free(p);
    } catch (...) {
    }
    p = nullptr;
    cap = 0;
  }

 public:
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  GrowBuf(GrowBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  GrowBuf& operator=(GrowBuf&& o) noexcept {
    if (this != &o) {
      drop();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~GrowBuf() { drop(); }

  void* data() const { return p; }
  size_t capacity() const { return cap; }

  // room for `bytes`, with a quarter of headroom when it has to grow (a
  // slightly larger call reuses the block); the contents are not kept
  void reserve(size_t bytes) {
    if (bytes > cap) regrow(bytes + bytes / 4);
  }
  void reserve_exact(size_t bytes) {
    if (bytes > cap) regrow(bytes);
  }
  // ... keeping the first `keep` bytes: the new block first, so a failed
  // allocation leaves the old block and its contents
  void reserve_keep(size_t bytes, size_t keep) {
    if (bytes <= cap) return;
    const size_t want = bytes + bytes / 4;
    void* q = Mem::alloc(want);
    if (keep) std::memcpy(q, p, keep);
    drop();
    p = q;
    cap = want;
  }
};

}  // namespace gsc
