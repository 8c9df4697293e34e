// par.hpp — the host thread pool of the library: parallel loops with the
// serial loop's results and errors, a parallel sort, and the upload image's
// host -> host copies.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <functional>
#include <mutex>
#include <vector>

namespace gsh {

// host threads of the encoder: GS_ENCODE_THREADS, else the CPUs this process
// may run on (sched_getaffinity) shared among LOCAL_WORLD_SIZE ranks of a
// torchrun job on the host, at most 16 (the GPU boxes give a process 16)
uint32_t enc_threads();

// the threads a par_for of n items in chunks of `grain` runs on (<= 1: the
// caller's loop), and that loop on the pool
uint32_t par_width(uint32_t n, uint32_t grain);
void par_run(uint32_t n, uint32_t grain, uint32_t T, std::function<void(uint32_t)> f);

// f(i) for every i in [0, n), chunks of `grain` handed out to up to
// enc_threads() threads; f must not throw (par_try)
template <class F>
void par_for(uint32_t n, uint32_t grain, F&& f) {
  const uint32_t T = par_width(n, grain);
  if (T <= 1) {
    for (uint32_t i = 0; i < n; i++) f(i);
    return;
  }
  par_run(n, grain, T, [&f](uint32_t i) { f(i); });
}

// par_for over an f that may throw: every item runs, and the exception of the
// lowest failing index is kept, the one the serial loop would raise
struct ParErr {
  uint32_t at;  // the failing index (n: none)
  std::exception_ptr err;
  void rethrow() const {
    if (err) std::rethrow_exception(err);
  }
};
template <class F>
ParErr par_try(uint32_t n, uint32_t grain, F&& f) {
  ParErr r{n, nullptr};
  std::mutex m;
  par_for(n, grain, [&](uint32_t i) {
    try {
      f(i);
    } catch (...) {
      std::lock_guard<std::mutex> g(m);
      if (i < r.at) r = ParErr{i, std::current_exception()};
    }
  });
  return r;
}

// g() on a pool worker, not waited for (the calling thread runs it itself
// when there are no workers, and under AddressSanitizer so that its leak
// check at exit sees no work in flight)
void run_detached(std::function<void()> g);

// v sorted by `less` (a strict weak order): chunks of at least 8192 elements
// sorted in parallel, then merged pairwise between two buffers; each merge is
// split into T output pieces by co-rank (merge path) so every round runs on
// all threads.  Under a total order the result is the one order whatever the
// split; elements that tie come out in an order that depends on it.  (Takes
// the vector, not iterators: the last round's buffer is swapped in.)
template <class V, class Less>
void par_sort(std::vector<V>& v, Less less) {
  const uint32_t n = (uint32_t)v.size();
  const uint32_t T = std::max<uint32_t>(1, std::min<uint32_t>(enc_threads(), n / 8192));
  std::vector<uint32_t> cut(T + 1);
  for (uint32_t t = 0; t <= T; t++) cut[t] = (uint32_t)((uint64_t)n * t / T);
  par_for(T, 1, [&](uint32_t t) { std::sort(v.begin() + cut[t], v.begin() + cut[t + 1], less); });
  std::vector<V> tmp(T > 1 ? n : 0);
  std::vector<V>* src = &v;
  std::vector<V>* dst = &tmp;
  for (uint32_t w = 1; w < T; w *= 2) {
    struct Piece {
      uint32_t a, m, b, k0, k1;
    };
    std::vector<Piece> pieces;
    for (uint32_t t = 0; t < T; t += 2 * w) {
      const uint32_t a = cut[t], m = cut[std::min(T, t + w)], b = cut[std::min(T, t + 2 * w)];
      for (uint32_t q = 0; q < T; q++)
        pieces.push_back({a, m, b, (uint32_t)((uint64_t)(b - a) * q / T), (uint32_t)((uint64_t)(b - a) * (q + 1) / T)});
    }
    const std::vector<V>& S = *src;
    std::vector<V>& D = *dst;
    // co-rank: how many of the output's first k come from the left run
    auto corank = [&](uint32_t a, uint32_t m, uint32_t b, uint32_t k) {
      uint32_t lo = k > b - m ? k - (b - m) : 0u, hi = std::min(k, m - a);
      while (lo < hi) {
        const uint32_t i = (lo + hi) / 2, j = k - i;  // i from the left, j from the right
        if (less(S[m + j - 1], S[a + i])) hi = i;    // right[j-1] < left[i]: take fewer from the left
        else lo = i + 1;
      }
      return lo;
    };
    par_for((uint32_t)pieces.size(), 1, [&](uint32_t x) {
      const Piece& pc = pieces[x];
      const uint32_t i0 = corank(pc.a, pc.m, pc.b, pc.k0), i1 = corank(pc.a, pc.m, pc.b, pc.k1);
      std::merge(S.begin() + pc.a + i0, S.begin() + pc.a + i1, S.begin() + pc.m + (pc.k0 - i0),
                 S.begin() + pc.m + (pc.k1 - i1), D.begin() + pc.a + pc.k0, less);
    });
    std::swap(src, dst);
  }
  if (src != &v) v.swap(tmp);
}

// host -> host copies of an upload image (gs_ctx::commit), split over the
// pool's threads when large
struct HostCopy {
  const void* src;
  size_t off, bytes;
};
void host_copy_parallel(void* dst_base, const HostCopy* copies, size_t n);

}  // namespace gsh
