// par.cpp — the host thread pool behind par.hpp.
#include "par.hpp"

#include <sched.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <system_error>
#include <thread>

namespace gsh {

uint32_t enc_threads() {
  static const uint32_t n = [] {
    if (const char* s = std::getenv("GS_ENCODE_THREADS")) {
      const int v = std::atoi(s);
      if (v >= 1) return (uint32_t)std::min(v, 64);
    }
    unsigned cpus = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) cpus = (unsigned)CPU_COUNT(&set);
    if (!cpus) cpus = std::thread::hardware_concurrency();
    if (const char* s = std::getenv("LOCAL_WORLD_SIZE")) {
      const int w = std::atoi(s);
      if (w > 1) cpus /= (unsigned)w;
    }
    return (uint32_t)std::max(1u, std::min(cpus ? cpus : 1u, 16u));
  }();
  return n;
}

namespace {

// One process-wide pool of enc_threads() - 1 workers (started on first use,
// never torn down) serves every par_for: a call posts tokens for its job and
// works on it itself, so it completes even when every worker is busy (nested
// or concurrent calls from several contexts' threads).  A forked child has
// no workers and runs its loops serially.
struct PoolJob {
  std::function<void(uint32_t)> f;
  uint32_t n = 0, grain = 1;
  std::atomic<uint32_t> next{0}, done{0};
  std::mutex m;
  std::condition_variable cv;
  void work() {
    for (;;) {
      const uint32_t b = next.fetch_add(grain);
      if (b >= n) break;
      const uint32_t e = std::min(n, b + grain);
      for (uint32_t i = b; i < e; i++) f(i);
      if (done.fetch_add(e - b) + (e - b) == n) {
        std::lock_guard<std::mutex> g(m);
        cv.notify_all();
      }
    }
  }
};
struct Pool {
  pid_t pid = getpid();
  std::mutex m;
  std::condition_variable cv;
  std::deque<std::shared_ptr<PoolJob>> tokens;
  uint32_t workers = 0;
  explicit Pool(uint32_t n) {
    for (uint32_t t = 0; t < n; t++) {
      try {
        std::thread([this] { loop(); }).detach();
        workers++;
      } catch (const std::system_error&) {
        break;  // fewer workers: callers still finish their own jobs
      }
    }
  }
  void loop() {
    for (;;) {
      std::shared_ptr<PoolJob> j;
      {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return !tokens.empty(); });
        j = std::move(tokens.front());
        tokens.pop_front();
      }
      j->work();
    }
  }
};
// the pool when it has workers this process may use (null: run serially)
Pool* pool() {
  static Pool* p = new Pool(enc_threads() - 1);  // intentionally never destroyed (workers block on it)
  return p->workers && p->pid == getpid() ? p : nullptr;
}

}  // namespace

uint32_t par_width(uint32_t n, uint32_t grain) {
  grain = std::max<uint32_t>(grain, 1);
  const uint32_t T = std::min<uint32_t>(enc_threads(), (n + grain - 1) / grain);
  return T > 1 && pool() ? T : 1;
}

void par_run(uint32_t n, uint32_t grain, uint32_t T, std::function<void(uint32_t)> f) {
  Pool* pl = pool();
  auto j = std::make_shared<PoolJob>();
  j->f = std::move(f);
  j->n = n;
  j->grain = std::max<uint32_t>(grain, 1);
  {
    std::lock_guard<std::mutex> g(pl->m);
    for (uint32_t t = 1; t < T && t <= pl->workers; t++) pl->tokens.push_back(j);
  }
  pl->cv.notify_all();
  j->work();
  std::unique_lock<std::mutex> g(j->m);
  j->cv.wait(g, [&] { return j->done.load() == n; });
}

void run_detached(std::function<void()> g) {
#if defined(__SANITIZE_ADDRESS__)
  g();
#else
  Pool* pl = enc_threads() > 1 ? pool() : nullptr;
  if (!pl) {
    g();
    return;
  }
  auto j = std::make_shared<PoolJob>();
  j->f = [g = std::move(g)](uint32_t) { g(); };
  j->n = 1;
  {
    std::lock_guard<std::mutex> l(pl->m);
    pl->tokens.push_back(j);
  }
  pl->cv.notify_one();
#endif
}

void host_copy_parallel(void* dst_base, const HostCopy* copies, size_t n) {
  // pieces of at most 1 MiB, handed out to the pool's threads
  constexpr size_t kPiece = 1u << 20;
  std::vector<HostCopy> pieces;
  size_t total = 0;
  for (size_t i = 0; i < n; i++)
    for (size_t o = 0; o < copies[i].bytes; o += kPiece)
      pieces.push_back({(const char*)copies[i].src + o, copies[i].off + o, std::min(kPiece, copies[i].bytes - o)});
  for (auto& p : pieces) total += p.bytes;
  char* dst = (char*)dst_base;
  par_for((uint32_t)pieces.size(), total >= (8u << 20) ? 1u : (uint32_t)pieces.size() + 1,
          [&](uint32_t i) { std::memcpy(dst + pieces[i].off, pieces[i].src, pieces[i].bytes); });
}

}  // namespace gsh
