// batch_common.hpp — what the batch families (batch.cpp: gs_batch_*,
// batch_consolidate.hip: gs_batch_consolidate_*) share: the slot, the state
// every batch keeps, and the host thread loop.  Group keys and group building,
// eligibility, the gathers, the run loops and the argument checks differ in
// substance and stay with their family.
#pragma once
#include <atomic>
#include <thread>

#include "ctx.hpp"

namespace gsc {

constexpr uint32_t kEncodeThreads = 16;

// fn(i) for every i < n on up to max_threads host threads, the caller among them
template <class F>
void parallel_for(uint32_t n, uint32_t max_threads, F fn) {
  std::atomic<uint32_t> next{0};
  auto work = [&] {
    for (;;) {
      const uint32_t i = next.fetch_add(1);
      if (i >= n) return;
      fn(i);
    }
  };
  std::vector<std::thread> th;
  const uint32_t nt = std::min(max_threads, n);
  for (uint32_t t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// A slot is a child gs_ctx (the state a prepare produces: encoding, arena,
// DevProblem, result storage) that borrows the parent's stream and events, so
// a batch of 4,096 slots holds no stream of its own; ~gs_ctx frees memory only.
struct SlotCore {
  gs_ctx* c = nullptr;
  gs_status status = GS_E_INVALID;
  bool fallback = false;  // solved by the slot's own launches, after the batched ones
};

inline gs_ctx* new_slot_ctx(const gs_ctx* parent) {
  gs_ctx* s = new gs_ctx();
  s->device = parent->device;
  s->cfg_flags = parent->cfg_flags;
  s->stream = parent->stream;
  std::copy(std::begin(parent->ev), std::end(parent->ev), std::begin(s->ev));
  return s;
}

template <class Slot>
struct BatchBase {
  std::vector<Slot> slots;  // only grows: a slot's arena and pinned staging are reused
  uint32_t n = 0;           // slots of the current batch
  bool prepared = false, ran = false;
  std::vector<uint32_t> order;  // device array position -> slot
  gs_batch_stats stats{};
  gs_batch_fetch_stats fstats{};
  DevBuf dev;        // the device array of the batched slots' problems
  DevBuf g_dev;      // fetch_all: the staging buffer ...
  PinnedBuf g_host;  // ... and its pinned mirror

  BatchBase() = default;
  BatchBase(const BatchBase&) = delete;
  BatchBase& operator=(const BatchBase&) = delete;
  ~BatchBase() {
    for (Slot& s : slots) delete s.c;
  }
  void ensure_slots(const gs_ctx* parent, uint32_t count) {
    while (slots.size() < count) {
      Slot s;
      s.c = new_slot_ctx(parent);
      slots.push_back(s);
    }
  }
  void copy_status(gs_status* status, uint32_t count) const {
    for (uint32_t i = 0; i < count; i++) status[i] = slots[i].status;
  }
};

// the bodies of gs_batch_*_last_run, _last_fetch and _error (b: the context's batch, or nullptr)
template <class B>
gs_status batch_last_run(const B* b, gs_batch_stats* out) {
  if (!b || !out || !b->prepared) return GS_E_INVALID;
  *out = b->stats;
  return GS_OK;
}
template <class B>
gs_status batch_last_fetch(const B* b, gs_batch_fetch_stats* out) {
  if (!b || !out || !b->prepared) return GS_E_INVALID;
  *out = b->fstats;
  return GS_OK;
}
template <class B>
size_t batch_error(const B* b, uint32_t i, char* buf, size_t len) {
  if (!b || i >= b->n) return 0;
  return gs_last_error(b->slots[i].c, buf, len);
}

}  // namespace gsc
