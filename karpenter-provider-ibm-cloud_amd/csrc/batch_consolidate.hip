// batch_consolidate.hip — gs_batch_consolidate_*: the consolidation
// simulations of many independent clusters on one context, in a number of
// device operations that does not depend on how many clusters they are.
//
// A slot is a child gs_ctx as in batch.cpp (batch_common.hpp: the slot core,
// the state every batch keeps, the host thread loop) holding what
// gs_consolidate leaves resident: the input copy, the encoding, the plan, the
// arena and the pinned result staging.  This unit holds what is the
// consolidation batch's own: group keys, eligibility, the run loop, the
// gather and its validation.
//
// Prepare runs gs_consolidate's host steps per slot (consolidate.cpp cons_*:
// check, take + encode and plan the sets on up to 16 host threads, then the
// grid plan and the upload one after another), copies the DevProblem structs
// of the slots with simulations into one device array ordered by group,
// followed by each slot's workgroup count, and that is the only copy: a run
// launches kernels only.
//
//  group     the slots that need the same instantiation of every kernel:
//            (R, general or not) of the simulation kernel, the lane-pair width
//            of K1/K2, and whether K3 runs the minValues form.  The shape
//            (FB_SIM / FB_SIM_NARROW) is one per batch, from the total number
//            of simulations.  Five launches per group (six with minValues):
//            cursors, rows, begin (work counters; overlay cells when the
//            stamp prefix wraps), simulations, truncation (+ settlement).
//  no launch a slot without simulations (no candidates, or all filtered by its
//            shard filter): its fetch decides an empty or all-SKIPPED table.
//  fallback  a slot whose simulations need more dynamic LDS than the batched
//            instantiations may use: cons_launch on the slot after the
//            batched launches.  The single kernel has the same static LDS, so
//            none is expected; the path keeps such a slot correct.
//  epoch     the overlay stamp prefix is the batch's and travels as a kernel
//            argument, so a run copies nothing; gs_batch_consolidate_results
//            draws the next prefix for its rerun, and when the prefix wraps
//            every group's overlay cells are cleared (one launch per group).
//  fetch_all every slot decided after one device pass: two launches per group
//            (batch_kernels.hip: settle, options) pack what the decisions read
//            into one staging buffer, which comes back in one transfer (two
//            the first time after a prepare); cons_decide_records then decides each slot from its
//            records, the code the per-slot fetch ends in too.
#include <tuple>

#include "batch_common.hpp"

namespace gsc {

struct ConsSlot : SlotCore {  // fallback: has simulations the batched launches do not cover
  bool grouped = false;  // in the device array: the batched launches cover it
  bool fetched = false;  // copied back and decided since the last run
  gs_status fetch_status = GS_OK;
};

struct ConsBatch : BatchBase<ConsSlot> {
  uint32_t nt = 256;   // the batch's simulation workgroup shape
  uint32_t epoch = 0;  // the last overlay stamp prefix drawn (1..4095)
  struct Group {
    uint32_t R, general, lp, mv;
    uint32_t first = 0, count = 0;  // range of the device array
    uint32_t lds = 0, max_blocks = 0, max_sims = 0, max_slots = 0, trunc_lds = 0;
    uint64_t max_cursors = 0, max_pairs = 0;
  };
  std::vector<Group> groups;
  // the device image (dev): order.size() DevProblem, then order.size() workgroup
  // counts, then each slot's first record in fetch_all's simulation table
  const gsd::DevProblem* problems() const { return (const gsd::DevProblem*)dev.data(); }
  const uint32_t* blocks() const { return (const uint32_t*)(problems() + order.size()); }
  const uint32_t* sim_base() const { return blocks() + order.size(); }
  // gs_batch_consolidate_fetch_all: the staging buffer (g_dev) and its pinned
  // mirror (g_host).  Layout: a 64-B head whose first word is the option
  // cursor, SlotOut[order.size()], SimOut[n_sims], then the option region
  // (60 per simulation on the device; the mirror holds what a call transfers).
  std::vector<uint32_t> h_sim_base;  // device array position -> first record
  uint64_t n_sims = 0;               // simulations of the grouped slots
  uint32_t opt_hint = 0;             // options the last fetch_all of this batch found: the next one's first transfer carries as many
};
constexpr size_t kGatherHead = 64;
// more simulations than the 32-bit option offsets address: no gathered path
constexpr uint64_t kGatherMaxSims = 1ull << 26;

namespace {

using GroupKey = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>;

GroupKey key_of(const gsh::Encoded& e) {
  return GroupKey{e.R, gsd::general_variant(e) ? 1u : 0u, gsk_feas_lp(e.W), e.any_mv ? 1u : 0u};
}

bool eligible(const ConsBatch& b, const ConsSlot& s) {
  const gsd::DevProblem& d = s.c->dp;
  return d.R >= 1 && d.R <= 8 && d.sim_nt == b.nt && gsd::sim_lds_bytes(d) <= gsk_ffd_sim_batch_dyn_lds_max();
}

// the device array of the slots with simulations, ordered by group, and their
// workgroup counts: one copy
void build_groups(gs_ctx* c, ConsBatch& b) {
  std::map<GroupKey, std::vector<uint32_t>> by;
  for (uint32_t i = 0; i < b.n; i++) {
    ConsSlot& s = b.slots[i];
    s.grouped = s.fallback = false;
    if (s.status != GS_OK || s.c->sims.evaluated.empty()) continue;
    if (eligible(b, s)) by[key_of(s.c->enc)].push_back(i);
    else s.fallback = true;
  }
  b.groups.clear();
  b.order.clear();
  b.h_sim_base.clear();
  b.n_sims = 0;
  b.opt_hint = 0;
  std::vector<gsd::DevProblem> problems;
  std::vector<uint32_t> blocks;
  for (auto& kv : by) {
    ConsBatch::Group g{};
    std::tie(g.R, g.general, g.lp, g.mv) = kv.first;
    g.first = (uint32_t)b.order.size();
    g.count = (uint32_t)kv.second.size();
    for (uint32_t i : kv.second) {
      ConsSlot& s = b.slots[i];
      const gsd::DevProblem& d = s.c->dp;
      const SimPlan& sp = s.c->sims;
      g.lds = std::max(g.lds, gsd::sim_lds_bytes(d));
      g.max_blocks = std::max(g.max_blocks, sp.blocks);
      g.max_sims = std::max(g.max_sims, d.n_sims);
      g.max_slots = std::max(g.max_slots, (uint32_t)sp.pods.size());
      g.trunc_lds = std::max(g.trunc_lds, trunc_lds_bytes(d.N));
      g.max_pairs = std::max<uint64_t>(g.max_pairs, (uint64_t)d.V * d.T);
      g.max_cursors = std::max<uint64_t>(g.max_cursors, (uint64_t)d.V * d.T * d.R);
      s.grouped = true;
      b.order.push_back(i);
      problems.push_back(d);
      blocks.push_back(sp.blocks);
      b.h_sim_base.push_back((uint32_t)b.n_sims);
      b.n_sims += d.n_sims;
    }
    b.groups.push_back(g);
  }
  const size_t n = b.order.size(), bytes = n * (sizeof(gsd::DevProblem) + 2 * sizeof(uint32_t));
  if (!n) return;
  b.dev.reserve(bytes);
  std::vector<char> image(bytes);
  std::memcpy(image.data(), problems.data(), n * sizeof(gsd::DevProblem));
  std::memcpy(image.data() + n * sizeof(gsd::DevProblem), blocks.data(), n * sizeof(uint32_t));
  // (meaningless past kGatherMaxSims simulations, where fetch_all does not gather)
  std::memcpy(image.data() + n * (sizeof(gsd::DevProblem) + sizeof(uint32_t)), b.h_sim_base.data(), n * sizeof(uint32_t));
  HIPCHK(hipMemcpyAsync(b.dev.data(), image.data(), bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
}

// the next overlay stamp prefix (next_overlay_epoch's rule for the batch);
// true when it wrapped: the cells of 4,095 launches ago could match again, so
// every group's are cleared before the prefix is used
bool next_epoch(ConsBatch& b) {
  b.epoch = (b.epoch + 1u) & 0xFFFu;
  if (b.epoch) return false;
  b.epoch = 1;
  return true;
}

gs_status fetch_slot(gs_ctx* c, ConsSlot& s, gs_consolidation_result* out) {
  if (!s.fetched) {
    if (hipSetDevice(c->device) != hipSuccess) return fail(s.c, GS_E_HIP, "hipSetDevice failed");
    s.fetch_status = cons_fetch_decide(s.c, out);
    s.fetched = true;
    return s.fetch_status;
  }
  if (s.fetch_status == GS_OK) cons_fill_result(s.c, out);
  return s.fetch_status;
}

// gs_batch_consolidate_fetch_all's device pass: every grouped slot's records in
// the pinned mirror.  A 64-B clear (the option cursor), two launches per group,
// and one transfer of the head, the slot and the simulation records and the
// options behind them.  How many options there are is the cursor's final
// value, known after the synchronisation: the transfer carries as many as the
// batch's last fetch_all found (a run on the same upload finds the same), and
// only when there are more, as in the first call after a prepare, a second
// transfer brings the rest.  Nothing here depends on how many slots there are.
struct Gathered {
  const gsd::SlotOut* slots = nullptr;  // [order.size()]
  const gsd::SimOut* recs = nullptr;    // [n_sims], slot at h_sim_base
  const gsd::OptPair* opts = nullptr;   // [n_opts], slot at SlotOut::opt_base
  uint32_t n_opts = 0;
};

Gathered gather_all(gs_ctx* c, ConsBatch& b, gs_batch_fetch_stats& fs) {
  const size_t ng = b.order.size();
  const size_t recs_off = kGatherHead + ng * sizeof(gsd::SlotOut);
  const size_t opts_off = recs_off + b.n_sims * sizeof(gsd::SimOut);
  const size_t dev_bytes = opts_off + b.n_sims * gsd::SIM_OPTS_MAX * sizeof(gsd::OptPair);
  b.g_dev.reserve(dev_bytes);
  // (the mirror grows to what a call transfers; reserve_keep's `keep` bytes of it survive)
  b.opt_hint = (uint32_t)std::min<uint64_t>(b.opt_hint, b.n_sims * gsd::SIM_OPTS_MAX);  // within the device region
  const size_t first = opts_off + (size_t)b.opt_hint * sizeof(gsd::OptPair);
  b.g_host.reserve_keep(first, 0);
  char* dev = (char*)b.g_dev.data();
  gsd::SlotOut* d_slots = (gsd::SlotOut*)(dev + kGatherHead);
  gsd::SimOut* d_recs = (gsd::SimOut*)(dev + recs_off);
  gsd::OptPair* d_opts = (gsd::OptPair*)(dev + opts_off);
  HIPCHK(hipMemsetAsync(dev, 0, kGatherHead, c->stream));
  HIPCHK(hipEventRecord(c->ev[6], c->stream));
  for (const ConsBatch::Group& g : b.groups)
    HIPCHK(gsk_cons_gather_batch(b.problems() + g.first, b.blocks() + g.first, b.sim_base() + g.first, g.count, g.max_sims,
                                 d_slots + g.first, d_recs, d_opts, (uint32_t*)dev, c->stream));
  HIPCHK(hipEventRecord(c->ev[7], c->stream));
  HIPCHK(hipMemcpyAsync(b.g_host.data(), dev, first, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  fs.n_launches = 1u + 2u * (uint32_t)b.groups.size();
  fs.n_copies = 1;
  fs.bytes = first;
  Gathered g;
  g.n_opts = *(const uint32_t*)b.g_host.data();
  if (g.n_opts > b.n_sims * gsd::SIM_OPTS_MAX) throw HipError{"gs_batch_consolidate_fetch_all: corrupt option count"};
  if (g.n_opts > b.opt_hint) {
    const size_t bytes = (size_t)(g.n_opts - b.opt_hint) * sizeof(gsd::OptPair);
    b.g_host.reserve_keep(first + bytes, first);
    HIPCHK(hipMemcpyAsync((char*)b.g_host.data() + first, d_opts + b.opt_hint, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    fs.n_copies++;
    fs.bytes += bytes;
  }
  b.opt_hint = g.n_opts;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
  fs.device_ms = ms;
  const char* host = (const char*)b.g_host.data();
  g.slots = (const gsd::SlotOut*)(host + kGatherHead);
  g.recs = (const gsd::SimOut*)(host + recs_off);
  g.opts = (const gsd::OptPair*)(host + opts_off);
  return g;
}

// a gathered slot's records address only the slot's own options
bool records_valid(const Gathered& g, const gsd::SlotOut& so, const gsd::SimOut* rec, size_t n) {
  if ((uint64_t)so.opt_base + so.n_opt > g.n_opts) return false;
  for (size_t k = 0; k < n; k++)
    if (rec[k].n_opt > gsd::SIM_OPTS_MAX || (uint64_t)rec[k].opt_off + rec[k].n_opt > so.n_opt) return false;
  return true;
}

}  // namespace

void batch_consolidate_destroy(gs_ctx* c) {
  delete c->cons_batch;  // its slots and buffers with it
  c->cons_batch = nullptr;
}

}  // namespace gsc

using namespace gsc;

extern "C" {

gs_status gs_batch_consolidate_prepare(gs_ctx* c, const gs_consolidation* const* in, uint32_t n, gs_status* status) {
  if (!c) return GS_E_INVALID;
  if (n && (!in || !status)) return fail(c, GS_E_INVALID, "gs_batch_consolidate_prepare: NULL inputs or status");
  if (!c->shards.empty())
    return fail(c, GS_E_INVALID, "gs_batch_consolidate_prepare: a context with shards runs no batch");
  if (n > GS_BATCH_MAX) return fail(c, GS_E_CAPACITY, "gs_batch_consolidate_prepare: more than 4096 inputs");
  const auto t0 = Clock::now();
  if (!c->cons_batch) c->cons_batch = new ConsBatch();
  ConsBatch& b = *c->cons_batch;
  b.prepared = b.ran = false;
  b.n = 0;
  b.groups.clear();
  b.order.clear();
  b.fstats = gs_batch_fetch_stats{};
  b.ensure_slots(c, n);
  // check, take + encode and plan the sets on up to 16 host threads (the
  // encoder's own loops share its pool)
  parallel_for(n, kEncodeThreads, [&](uint32_t i) {
    ConsSlot& s = b.slots[i];
    gs_ctx* sc = s.c;
    sc->prepared = sc->ran = false;
    sc->cons_ready = false;
    sc->err.clear();
    sc->sims = SimPlan{};
    sc->commands.clear();
    s.grouped = s.fallback = s.fetched = false;
    s.fetch_status = GS_OK;
    std::string err;
    s.status = cons_check_input(in[i], &err);
    if (s.status != GS_OK) {
      fail(sc, s.status, err);
      return;
    }
    s.status = cons_take_input(sc, in[i]);
    if (s.status != GS_OK) return;
    s.status = cons_plan_sets(sc, &err);
    if (s.status != GS_OK) fail(sc, s.status, err);
  });
  // the batch's shape from all its simulations, each slot's share of its
  // group's resident workgroups, then the uploads and the device array
  uint32_t accepted = 0;
  try {
    HIPCHK(hipSetDevice(c->device));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    size_t total = 0;
    std::map<GroupKey, uint64_t> group_sims;
    for (uint32_t i = 0; i < n; i++) {
      const ConsSlot& s = b.slots[i];
      if (s.status != GS_OK) continue;
      total += s.c->sims.evaluated.size();
      group_sims[key_of(s.c->enc)] += s.c->sims.evaluated.size();
    }
    b.nt = cons_sim_threads(total, cus);
    for (uint32_t i = 0; i < n; i++) {
      ConsSlot& s = b.slots[i];
      if (s.status != GS_OK) continue;
      std::string err;
      const SimBudget budget{b.nt, group_sims[key_of(s.c->enc)]};
      s.status = cons_plan_grid(s.c, &budget, &err);
      if (s.status != GS_OK) {
        fail(s.c, s.status, err);
        continue;
      }
      const gs_status up = cons_upload(s.c);
      if (up != GS_OK) throw HipError{"slot " + std::to_string(i) + ": " + s.c->err};
      accepted++;
    }
    b.n = n;
    build_groups(c, b);
  } catch (const HipError& e) {
    b.copy_status(status, n);
    return fail(c, GS_E_HIP, e.msg);
  }
  b.copy_status(status, n);
  b.prepared = true;
  b.stats = gs_batch_stats{};
  b.stats.n_problems = n;
  b.stats.n_accepted = accepted;
  b.stats.prepare_ms = ms_since(t0);
  return GS_OK;
}

gs_status gs_batch_consolidate_run(gs_ctx* c) {
  if (!c || !c->cons_batch || !c->cons_batch->prepared) return GS_E_INVALID;
  ConsBatch& b = *c->cons_batch;
  const auto tw = Clock::now();
  uint32_t launches = 0, n_batched = 0, n_fallback = 0;
  float dev_ms = 0;
  b.ran = false;
  try {
    HIPCHK(hipSetDevice(c->device));
    if (!b.groups.empty()) {
      const uint32_t wrapped = next_epoch(b) ? 1u : 0u;
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      for (const ConsBatch::Group& g : b.groups) {
        const gsd::DevProblem* ds = b.problems() + g.first;
        const uint32_t* blk = b.blocks() + g.first;
        HIPCHK(gsk_feas_batch(ds, g.count, g.lp, g.max_cursors, g.max_pairs, c->stream));
        HIPCHK(gsk_sim_begin_batch(ds, blk, g.count, wrapped, c->stream));
        HIPCHK(gsk_ffd_sim_batch(ds, blk, g.count, g.max_blocks, g.R, g.general, b.nt, g.lds, b.epoch, c->stream));
        HIPCHK(gsk_trunc_sims_batch(ds, g.count, g.mv, g.max_sims, g.max_slots, g.trunc_lds, c->stream));
        launches += g.mv ? 6u : 5u;
      }
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      HIPCHK(hipEventSynchronize(c->ev[7]));
      HIPCHK(hipEventElapsedTime(&dev_ms, c->ev[6], c->ev[7]));
    }
  } catch (const HipError& e) {
    for (uint32_t i : b.order) reset_sim_counts(b.slots[i].c);
    return fail(c, GS_E_HIP, e.msg);
  }
  for (uint32_t i = 0; i < b.n; i++) {
    ConsSlot& s = b.slots[i];
    if (s.status != GS_OK) continue;
    gs_ctx* sc = s.c;
    s.fetched = false;
    s.fetch_status = GS_OK;
    if (s.fallback) {
      const gs_status st = cons_launch(sc);
      if (st != GS_OK) return fail(c, st, "slot " + std::to_string(i) + ": " + sc->err);
      n_fallback++;
      continue;
    }
    // covered by the batched launches, or without simulations (no launch)
    sc->t_feas = sc->t_sim = sc->t_trunc = 0;
    if (s.grouped) sc->dp.ov_epoch = b.epoch;
    n_batched++;
  }
  b.ran = true;
  b.stats.n_batched = n_batched;
  b.stats.n_fallback = n_fallback;
  b.stats.n_groups = (uint32_t)b.groups.size();
  b.stats.n_launches = launches;
  b.stats.device_ms = dev_ms;
  b.stats.run_ms = ms_since(tw);
  return GS_OK;
}

gs_status gs_batch_consolidate_fetch(gs_ctx* c, uint32_t i, gs_consolidation_result* out) {
  if (!c || !out || !c->cons_batch || !c->cons_batch->prepared || i >= c->cons_batch->n) return GS_E_INVALID;
  ConsSlot& s = c->cons_batch->slots[i];
  if (s.status != GS_OK) return s.status;
  if (!c->cons_batch->ran) return GS_E_INVALID;
  return fetch_slot(c, s, out);
}

gs_status gs_batch_consolidate_results(gs_ctx* c, uint32_t i, uint32_t sim, gs_result* out) {
  if (!c || !out || !c->cons_batch || !c->cons_batch->prepared || i >= c->cons_batch->n) return GS_E_INVALID;
  ConsBatch& b = *c->cons_batch;
  ConsSlot& s = b.slots[i];
  if (s.status != GS_OK) return s.status;
  if (!b.ran) return GS_E_INVALID;
  // the rerun overwrites what the fetch copies back: decide the slot first
  gs_consolidation_result table;
  const gs_status fs = fetch_slot(c, s, &table);
  if (fs != GS_OK) return fs;
  gs_ctx* sc = s.c;
  if (sim >= sc->commands.size()) return fail(sc, GS_E_INVALID, "simulation index out of range");
  if (sc->commands[sim].decision == GS_DECISION_SKIPPED)
    return fail(sc, GS_E_INVALID, "simulation skipped by the shard filter");
  if (s.grouped) {
    try {
      HIPCHK(hipSetDevice(c->device));
      if (next_epoch(b))
        for (const ConsBatch::Group& g : b.groups)
          HIPCHK(gsk_sim_begin_batch(b.problems() + g.first, b.blocks() + g.first, g.count, 1u, c->stream));
    } catch (const HipError& e) {
      return fail(sc, GS_E_HIP, e.msg);
    }
    sc->dp.ov_epoch = b.epoch - 1u;  // cons_sim_results draws the next one: the batch's
  }
  return cons_sim_results(sc, sim, out);
}

gs_status gs_batch_consolidate_fetch_all(gs_ctx* c, gs_consolidation_result* out, gs_status* status) {
  if (!c || !c->cons_batch || !c->cons_batch->prepared) return GS_E_INVALID;
  ConsBatch& b = *c->cons_batch;
  if (b.n && (!out || !status)) return fail(c, GS_E_INVALID, "gs_batch_consolidate_fetch_all: NULL out or status");
  if (!b.ran) return fail(c, GS_E_INVALID, "gs_batch_consolidate_fetch_all: the batch has not run");
  const auto t0 = Clock::now();
  gs_batch_fetch_stats fs{};
  fs.n_slots = b.n;
  std::vector<uint32_t> pos_of(b.n, 0);
  bool pending = false;
  for (uint32_t p = 0; p < b.order.size(); p++) {
    pos_of[b.order[p]] = p;
    pending = pending || !b.slots[b.order[p]].fetched;
  }
  b.copy_status(status, b.n);
  if (b.n) std::memset(out, 0, (size_t)b.n * sizeof(*out));
  Gathered g;
  bool gathered = false;
  if (pending && b.n_sims <= kGatherMaxSims) {
    try {
      HIPCHK(hipSetDevice(c->device));
      g = gather_all(c, b, fs);
      gathered = true;
    } catch (const HipError& e) {
      return fail(c, GS_E_HIP, e.msg);
    }
  }
  for (uint32_t i = 0; i < b.n; i++) {
    ConsSlot& s = b.slots[i];
    if (s.status != GS_OK) continue;
    if (!s.fetched && s.grouped && gathered) {
      const uint32_t p = pos_of[i];
      const gsd::SlotOut& so = g.slots[p];
      const gsd::SimOut* rec = g.recs + b.h_sim_base[p];
      if (records_valid(g, so, rec, s.c->sims.evaluated.size()))
        s.fetch_status = cons_decide_records(s.c, rec, g.opts + so.opt_base, so);
      else
        s.fetch_status = fail(s.c, GS_E_HIP, "gs_batch_consolidate_fetch_all: corrupt simulation records");
      s.fetched = true;
      status[i] = s.fetch_status;
      fs.n_decided++;
      continue;
    }
    // no gather: a slot without simulations (no device operation), a fallback
    // slot, or one fetched since the run (its table is kept)
    if (!s.fetched && !s.c->sims.evaluated.empty()) {
      const size_t ns = s.c->sims.evaluated.size();
      fs.n_copies += 5;
      fs.bytes += ns * (sizeof(gsd::SimCtrl) + sizeof(gsd::ClaimRec) + 61 * sizeof(uint32_t)) +
                  s.c->sims.blocks * sizeof(gsd::Ctrl);
    }
    gs_consolidation_result table;
    status[i] = fetch_slot(c, s, &table);
    fs.n_per_slot++;
  }
  fs.wall_ms = ms_since(t0);
  for (uint32_t i = 0; i < b.n; i++) {
    if (status[i] != GS_OK) continue;
    gs_ctx* sc = b.slots[i].c;
    sc->t_fetch = fs.wall_ms;
    cons_fill_result(sc, &out[i]);
  }
  b.fstats = fs;
  return GS_OK;
}

gs_status gs_batch_consolidate_last_fetch(const gs_ctx* c, gs_batch_fetch_stats* out) {
  return batch_last_fetch(c ? c->cons_batch : nullptr, out);
}

uint32_t gs_batch_fetch_stats_size(void) { return (uint32_t)sizeof(gs_batch_fetch_stats); }

size_t gs_batch_consolidate_error(const gs_ctx* c, uint32_t i, char* buf, size_t len) {
  return batch_error(c ? c->cons_batch : nullptr, i, buf, len);
}

gs_status gs_batch_consolidate_last_run(const gs_ctx* c, gs_batch_stats* out) {
  return batch_last_run(c ? c->cons_batch : nullptr, out);
}

}  // extern "C"
