// batch.cpp — gs_batch_*: many independent provisioning Solves on one
// context, one workgroup each, in a number of kernel launches that does not
// depend on how many they are.
//
// A slot is a child gs_ctx (the state prepare_one produces: encoding, arena,
// DevProblem, result storage) that borrows the parent's stream and events, so
// a batch of 4,096 slots holds no stream of its own.  The problems are encoded
// on up to 16 host threads and uploaded one after another; the DevProblem
// structs of the batch-eligible slots are then copied into one device array,
// ordered by group, and every kernel of the Solve path reads its problem from
// that array (batch_kernels.hip, ffd_wave_batch_r.hip).
//
//  eligible  the single-wave kernel with its claim state in LDS, on a context
//            with neither GS_CFG_BLOCK_SOLVE nor GS_CFG_CLAIMS_HBM
//  fallback  every other accepted slot: gs_run on the slot, after the batched
//            launches.  A batched slot that opens more NodeClaims than its
//            LDS holds (ST_CLAIMS) reruns through gs_run's grow-and-rerun
//            path and stays a fallback slot.
//  group     the eligible slots that need the same instantiation of every
//            kernel: (R, TOPO, WIDE) of K4 and the lane-pair width of K1/K2.
//            Five launches per group: cursors, rows, state reset, Solve,
//            truncation.
#include <atomic>
#include <thread>
#include <tuple>

#include "ctx.hpp"

extern "C" uint32_t gsk_ffdw_wide(uint32_t W);

namespace gsc {

struct BatchSlot {
  gs_ctx* c = nullptr;
  gs_status status = GS_E_INVALID;
  bool fallback = false;  // solved through gs_run
};

struct Batch {
  std::vector<BatchSlot> slots;  // only grows: a slot's arena and pinned staging are reused
  uint32_t n = 0;                // slots of the current batch
  bool prepared = false, ran = false;
  bool dirty = true;             // the device array is out of date (a prepare, or a slot turned fallback)
  struct Group {
    uint32_t R, topo, wide, lp;
    uint32_t first = 0, count = 0;  // range of the device array
    uint32_t lds = 0, max_slots = 0, trunc_lds = 0;
    uint64_t max_cursors = 0, max_pairs = 0;
  };
  std::vector<Group> groups;
  std::vector<uint32_t> order;       // device array position -> slot
  std::vector<gsd::DevProblem> host; // the array's host image
  gsd::DevProblem* dev = nullptr;
  size_t dev_cap = 0;
  gs_batch_stats stats{};
};

namespace {

constexpr uint32_t kLaunchesPerGroup = 5;
constexpr uint32_t kEncodeThreads = 16;

void free_slot(gs_ctx* s) {
  s->free_all();
  if (s->arena) (void)hipFree(s->arena);
  if (s->stage) (void)hipHostFree(s->stage);
  delete s;  // the stream and the events are the parent's
}

// the dynamic LDS gsk_ffdw requests for a problem with its claim state in LDS
uint32_t wave_lds(const gsd::DevProblem& d) {
  return gsk_ffd_lds_bytes(d.max_claims_wave, d.n_thr, 0, gsd::topo_lds_bytes(d.TGZ, d.ZS, d.TGH, d.n_lazy)) +
         gsd::wave_node_lds_bytes(d.NN);
}

bool eligible(const gs_ctx* parent, const BatchSlot& s) {
  if (s.status != GS_OK || s.fallback) return false;
  if (parent->cfg_flags & (GS_CFG_BLOCK_SOLVE | GS_CFG_CLAIMS_HBM)) return false;
  const gs_ctx* c = s.c;
  return c->wave && !c->ch && c->dp.R >= 1 && c->dp.R <= 8 && wave_lds(c->dp) <= gsk_ffdw_batch_dyn_lds_max();
}

void copy_to_device(gs_ctx* c, Batch& b, size_t n) {
  if (n > b.dev_cap) {
    if (b.dev) HIPCHK(hipFree(b.dev));
    b.dev = nullptr;
    b.dev_cap = 0;
    const size_t want = n + n / 4;
    HIPCHK(hipMalloc((void**)&b.dev, want * sizeof(gsd::DevProblem)));
    b.dev_cap = want;
  }
  if (n) {
    HIPCHK(hipMemcpyAsync(b.dev, b.host.data(), n * sizeof(gsd::DevProblem), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
}

// the device array of the eligible slots, ordered by group
void build_groups(gs_ctx* c, Batch& b) {
  using Key = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>;
  std::map<Key, std::vector<uint32_t>> by;
  for (uint32_t i = 0; i < b.n; i++) {
    const BatchSlot& s = b.slots[i];
    if (!eligible(c, s)) continue;
    const gsd::DevProblem& d = s.c->dp;
    const uint32_t topo = (d.TG || d.any_mv || d.any_vol) ? 1u : 0u;
    by[Key{d.R, topo, gsk_ffdw_wide(d.W), gsk_feas_lp(d.W)}].push_back(i);
  }
  b.groups.clear();
  b.order.clear();
  b.host.clear();
  for (auto& kv : by) {
    Batch::Group g{};
    std::tie(g.R, g.topo, g.wide, g.lp) = kv.first;
    g.first = (uint32_t)b.order.size();
    g.count = (uint32_t)kv.second.size();
    for (uint32_t i : kv.second) {
      const gsd::DevProblem& d = b.slots[i].c->dp;
      g.lds = std::max(g.lds, wave_lds(d));
      g.max_slots = std::max(g.max_slots, d.claim_cap);
      g.trunc_lds = std::max(g.trunc_lds, trunc_lds_bytes(d.N));
      g.max_pairs = std::max<uint64_t>(g.max_pairs, (uint64_t)d.V * d.T);
      g.max_cursors = std::max<uint64_t>(g.max_cursors, (uint64_t)d.V * d.T * d.R);
      b.order.push_back(i);
      b.host.push_back(d);
    }
    b.groups.push_back(g);
  }
  copy_to_device(c, b, b.host.size());
  b.dirty = false;
}

}  // namespace

void batch_destroy(gs_ctx* c) {
  Batch* b = c->batch;
  if (!b) return;
  for (auto& s : b->slots)
    if (s.c) free_slot(s.c);
  if (b->dev) (void)hipFree(b->dev);
  delete b;
  c->batch = nullptr;
}

}  // namespace gsc

using namespace gsc;

extern "C" {

uint32_t gs_batch_stats_size(void) { return (uint32_t)sizeof(gs_batch_stats); }

gs_status gs_batch_prepare(gs_ctx* c, const gs_problem* const* problems, uint32_t n, gs_status* status) {
  if (!c) return GS_E_INVALID;
  if (n && (!problems || !status)) return fail(c, GS_E_INVALID, "gs_batch_prepare: NULL problems or status");
  if (!c->shards.empty()) return fail(c, GS_E_INVALID, "gs_batch_prepare: a context with shards runs no batch");
  if (n > GS_BATCH_MAX) return fail(c, GS_E_CAPACITY, "gs_batch_prepare: more than 4096 problems");
  const auto t0 = Clock::now();
  if (!c->batch) c->batch = new Batch();
  Batch& b = *c->batch;
  b.prepared = b.ran = false;
  b.dirty = true;
  b.n = 0;
  while (b.slots.size() < n) {
    BatchSlot s;
    s.c = new gs_ctx();
    s.c->device = c->device;
    s.c->cfg_flags = c->cfg_flags;
    s.c->stream = c->stream;
    std::copy(std::begin(c->ev), std::end(c->ev), std::begin(s.c->ev));
    b.slots.push_back(s);
  }
  // encode on up to 16 host threads (the encoder's own loops share its pool)
  std::atomic<uint32_t> next{0};
  auto work = [&] {
    for (;;) {
      const uint32_t i = next.fetch_add(1);
      if (i >= n) return;
      BatchSlot& s = b.slots[i];
      gs_ctx* sc = s.c;
      sc->prepared = sc->ran = false;
      sc->cons_ready = false;
      sc->err.clear();
      s.fallback = false;
      if (!problems[i]) {
        s.status = fail(sc, GS_E_INVALID, "NULL problem");
        continue;
      }
      const auto te = Clock::now();
      gsh::Err er = gsh::encode(problems[i], sc->enc);
      sc->t_encode = ms_since(te);
      if (er.code == GS_OK) er = capacity_check(sc->enc);
      s.status = er.code == GS_OK ? GS_OK : fail(sc, er.code, er.msg);
      sc->n_nodepools = problems[i]->n_nodepools;
    }
  };
  {
    std::vector<std::thread> th;
    const uint32_t nt = std::min<uint32_t>(kEncodeThreads, n);
    for (uint32_t t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
  }
  // upload the accepted slots, then gather every slot's first-pass queue
  // records in one launch
  uint32_t accepted = 0;
  try {
    HIPCHK(hipSetDevice(c->device));
    std::vector<gsd::DevProblem>& all = b.host;
    all.clear();
    uint32_t max_pods = 0;
    for (uint32_t i = 0; i < n; i++) {
      BatchSlot& s = b.slots[i];
      if (s.status != GS_OK) continue;
      const auto tu = Clock::now();
      try {
        upload_problem(s.c, nullptr, false);
      } catch (const HipError& e) {
        // a slot's own capacity (no LDS left for NodeClaims) is the slot's; anything else is the call's
        if (e.msg.find("leaves no LDS") == std::string::npos) throw;
        s.status = fail(s.c, GS_E_CAPACITY, e.msg);
        continue;
      }
      s.c->t_upload = ms_since(tu);
      s.c->prepared = true;
      s.fallback = !eligible(c, s);
      all.push_back(s.c->dp);
      max_pods = std::max(max_pods, s.c->dp.P);
      accepted++;
    }
    copy_to_device(c, b, all.size());
    HIPCHK(gsk_queue_records_batch(b.dev, (uint32_t)all.size(), max_pods, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } catch (const HipError& e) {
    for (uint32_t i = 0; i < n; i++) status[i] = b.slots[i].status;
    return fail(c, GS_E_HIP, e.msg);
  }
  for (uint32_t i = 0; i < n; i++) status[i] = b.slots[i].status;
  b.n = n;
  b.prepared = true;
  b.stats = gs_batch_stats{};
  b.stats.n_problems = n;
  b.stats.n_accepted = accepted;
  b.stats.prepare_ms = ms_since(t0);
  return GS_OK;
}

gs_status gs_batch_run(gs_ctx* c) {
  if (!c || !c->batch || !c->batch->prepared) return GS_E_INVALID;
  Batch& b = *c->batch;
  const auto tw = Clock::now();
  uint32_t launches = 0, n_groups = 0, n_batched = 0, n_fallback = 0;
  float dev_ms = 0;
  try {
    HIPCHK(hipSetDevice(c->device));
    if (b.dirty) build_groups(c, b);
    n_groups = (uint32_t)b.groups.size();
    if (!b.groups.empty()) {
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      for (const Batch::Group& g : b.groups) {
        const gsd::DevProblem* ds = b.dev + g.first;
        HIPCHK(gsk_feas_batch(ds, g.count, g.lp, g.max_cursors, g.max_pairs, c->stream));
        HIPCHK(gsk_init_state_batch(ds, g.count, c->stream));
        HIPCHK(gsk_ffdw_batch(ds, g.count, g.R, g.topo, g.wide, g.lds, c->stream));
        HIPCHK(gsk_trunc_batch(ds, g.count, g.max_slots, g.trunc_lds, c->stream));
        launches += kLaunchesPerGroup;
      }
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      HIPCHK(hipEventSynchronize(c->ev[7]));
      HIPCHK(hipEventElapsedTime(&dev_ms, c->ev[6], c->ev[7]));
    }
    // a batched slot that can open more NodeClaims than its LDS holds may have
    // ended with ST_CLAIMS: it reruns alone (gs_run grows its claim arrays)
    // and stays a fallback slot
    for (uint32_t i : b.order) {
      BatchSlot& s = b.slots[i];
      gs_ctx* sc = s.c;
      sc->t_feas = sc->t_ffd = sc->t_trunc = sc->t_run_wall = 0;
      sc->ran = true;
      if (sc->dp.P > sc->dp.max_claims_wave) {
        uint32_t st = 0;
        HIPCHK(hipMemcpy(&st, &sc->dp.ctrl->status, sizeof st, hipMemcpyDeviceToHost));
        if (st == gsd::ST_CLAIMS) {
          s.fallback = true;
          b.dirty = true;
          continue;
        }
      }
      n_batched++;
    }
    for (uint32_t i = 0; i < b.n; i++) {
      BatchSlot& s = b.slots[i];
      if (s.status != GS_OK || !s.fallback) continue;
      const gs_status st = gs_run(s.c);
      if (st != GS_OK) return fail(c, st, "slot " + std::to_string(i) + ": " + s.c->err);
      n_fallback++;
    }
  } catch (const HipError& e) {
    return fail(c, GS_E_HIP, e.msg);
  }
  b.ran = true;
  b.stats.n_batched = n_batched;
  b.stats.n_fallback = n_fallback;
  b.stats.n_groups = n_groups;
  b.stats.n_launches = launches;
  b.stats.device_ms = dev_ms;
  b.stats.run_ms = ms_since(tw);
  return GS_OK;
}

gs_status gs_batch_fetch(gs_ctx* c, uint32_t i, gs_result* out) {
  if (!c || !out || !c->batch || !c->batch->prepared || i >= c->batch->n) return GS_E_INVALID;
  BatchSlot& s = c->batch->slots[i];
  if (s.status != GS_OK) return s.status;
  if (!c->batch->ran) return GS_E_INVALID;
  return gs_fetch(s.c, out);
}

size_t gs_batch_error(const gs_ctx* c, uint32_t i, char* buf, size_t len) {
  if (!c || !c->batch || i >= c->batch->n) return 0;
  return gs_last_error(c->batch->slots[i].c, buf, len);
}

gs_status gs_batch_last_run(const gs_ctx* c, gs_batch_stats* out) {
  if (!c || !out || !c->batch || !c->batch->prepared) return GS_E_INVALID;
  *out = c->batch->stats;
  return GS_OK;
}

}  // extern "C"
