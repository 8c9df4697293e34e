// growbuf_harness.cpp — GrowBuf (csrc/growbuf.hpp), the owner of every
// grow-only device buffer and pinned mirror of the library, on the CPU for a
// sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined tools/growbuf_harness.cpp
// It includes that header and nothing else of the library.
//
// usage: growbuf_harness <case>
// The memory policy is malloc-backed and records every call: 'a' an
// allocation, 'x' an allocation told to throw, 'f' a free.  A double free, a
// leak or a read of a freed block is a sanitizer report.  Output: one line of
// key=value facts about the case, which tests/test_growbuf.py asserts.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <utility>

#include "../karpenter-provider-ibm-cloud_amd/csrc/growbuf.hpp"

namespace {

struct TestMem {
  static std::string events;  // calls in order
  static std::string sizes;   // bytes of each successful allocation, comma-separated
  static int alloc_calls;
  static int fail_alloc_at;   // the k-th allocation call throws (1-based; 0: none)
  static int free_throws;     // 1: a free releases the block, then reports an error; 2: it reports one and releases nothing
  static void* alloc(size_t n) {
    if (++alloc_calls == fail_alloc_at) {
      events += 'x';
      throw std::runtime_error("alloc");
    }
    events += 'a';
    sizes += (sizes.empty() ? "" : ",") + std::to_string(n);
    return std::malloc(n);
  }
  static void free(void* p) {
    events += 'f';
    if (free_throws != 2) std::free(p);
    if (free_throws) throw std::runtime_error("free");
  }
};
std::string TestMem::events, TestMem::sizes;
int TestMem::alloc_calls = 0, TestMem::fail_alloc_at = 0;
int TestMem::free_throws = 0;

using Buf = gsc::GrowBuf<TestMem>;

void fill(Buf& b, size_t n, unsigned seed) {
  for (size_t i = 0; i < n; i++) ((unsigned char*)b.data())[i] = (unsigned char)(i * 131u + seed);
}
bool holds(const Buf& b, size_t n, unsigned seed) {
  for (size_t i = 0; i < n; i++)
    if (((const unsigned char*)b.data())[i] != (unsigned char)(i * 131u + seed)) return false;
  return true;
}
const char* ev() { return TestMem::events.empty() ? "-" : TestMem::events.c_str(); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: growbuf_harness <case>\n");
    return 2;
  }
  const std::string c = argv[1];
  if (c == "reserve" || c == "reserve_exact") {
    const bool exact = c == "reserve_exact";
    auto grow = [&](Buf& b, size_t n) { exact ? b.reserve_exact(n) : b.reserve(n); };
    std::string within;
    size_t cap1 = 0;
    {
      Buf b;
      grow(b, 100);
      cap1 = b.capacity();
      fill(b, cap1, 1);  // the whole capacity is the buffer's to write
      grow(b, cap1);
      grow(b, 50);
      grow(b, 0);
      within = ev();
      grow(b, cap1 + 1);
      fill(b, b.capacity(), 2);
      std::printf("within=%s cap1=%zu cap2=%zu ", within.c_str(), cap1, b.capacity());
    }
    std::printf("events=%s sizes=%s\n", ev(), TestMem::sizes.c_str());
    return 0;
  }
  if (c == "zero") {
    Buf b;
    b.reserve(0);
    b.reserve_exact(0);
    b.reserve_keep(0, 0);
    std::printf("events=%s null=%d cap=%zu\n", ev(), b.data() == nullptr, b.capacity());
    return 0;
  }
  if (c == "alloc_throws") {
    int caught = 0, null_after = 0;
    size_t cap_after = 1, cap_later = 0;
    {
      Buf b;
      b.reserve(100);
      TestMem::fail_alloc_at = 2;
      try {
        b.reserve(200);
      } catch (const std::runtime_error&) {
        caught = 1;
      }
      null_after = b.data() == nullptr;
      cap_after = b.capacity();
      b.reserve(10);
      fill(b, b.capacity(), 3);
      cap_later = b.capacity();
    }
    std::printf("caught=%d null=%d cap=%zu later=%zu events=%s\n", caught, null_after, cap_after, cap_later, ev());
    return 0;
  }
  if (c == "keep") {
    int kept = 0, caught = 0, same = 0, intact = 0;
    size_t cap2 = 0, cap3 = 0;
    std::string grown;
    {
      Buf b;
      b.reserve_keep(64, 0);
      fill(b, 64, 4);
      b.reserve_keep(64, 64);  // within capacity: no call
      b.reserve_keep(200, 64);
      kept = holds(b, 64, 4);
      cap2 = b.capacity();
      grown = ev();
      fill(b, cap2, 5);
      const void* before = b.data();
      TestMem::fail_alloc_at = TestMem::alloc_calls + 1;
      try {
        b.reserve_keep(1000, 200);
      } catch (const std::runtime_error&) {
        caught = 1;
      }
      same = b.data() == before;
      cap3 = b.capacity();
      intact = holds(b, cap2, 5);
    }
    std::printf("kept=%d cap2=%zu grown=%s caught=%d same=%d cap3=%zu intact=%d events=%s sizes=%s\n", kept, cap2,
                grown.c_str(), caught, same, cap3, intact, ev(), TestMem::sizes.c_str());
    return 0;
  }
  if (c == "move") {
    int a_empty = 0, b_took = 0, b_empty = 0, c_took = 0;
    std::string assigned, constructed;
    {
      Buf a, b;
      a.reserve_exact(10);
      b.reserve_exact(20);
      fill(a, 10, 6);
      const void* pa = a.data();
      b = std::move(a);
      assigned = ev();
      a_empty = a.data() == nullptr && a.capacity() == 0;
      b_took = b.data() == pa && b.capacity() == 10 && holds(b, 10, 6);
      Buf d(std::move(b));
      constructed = ev();
      b_empty = b.data() == nullptr && b.capacity() == 0;
      c_took = d.data() == pa && d.capacity() == 10 && holds(d, 10, 6);
    }
    std::printf("assigned=%s constructed=%s a_empty=%d b_took=%d b_empty=%d c_took=%d events=%s\n", assigned.c_str(),
                constructed.c_str(), a_empty, b_took, b_empty, c_took, ev());
    return 0;
  }
  if (c == "free_throws") {
    // reserve reports the free's error and still owns the block; the destructor
    // and move-assignment ignore it
    int caught = 0, owned = 0;
    {
      Buf d;
      d.reserve_exact(10);
      fill(d, 10, 7);
      TestMem::free_throws = 2;
      try {
        d.reserve(100);
      } catch (const std::runtime_error&) {
        caught = 1;
      }
      owned = d.capacity() == 10 && holds(d, 10, 7);
      TestMem::free_throws = 0;
      d.reserve(100);
      Buf a, b;
      a.reserve(10);
      b.reserve(10);
      TestMem::free_throws = 1;
      a = std::move(b);
    }
    std::printf("survived=1 caught=%d owned=%d events=%s\n", caught, owned, ev());
    return 0;
  }
  if (c == "up256") {
    static_assert(gsc::up256(0) == 0 && gsc::up256(1) == 256 && gsc::up256(255) == 256, "up256 below");
    static_assert(gsc::up256(256) == 256 && gsc::up256(257) == 512, "up256 at and above");
    std::printf("%zu %zu %zu %zu %zu\n", gsc::up256(0), gsc::up256(1), gsc::up256(255), gsc::up256(256), gsc::up256(257));
    return 0;
  }
  std::fprintf(stderr, "unknown case %s\n", c.c_str());
  return 2;
}
