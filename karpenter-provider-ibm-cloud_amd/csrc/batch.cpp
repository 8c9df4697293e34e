// batch.cpp — gs_batch_*: many independent provisioning Solves on one
// context, one workgroup each, in a number of kernel launches that does not
// depend on how many they are.
//
// A slot is a child gs_ctx (the state prepare_one produces) on the parent's
// stream and events.  The slot, the state every batch keeps and the host
// thread loop are batch_common.hpp's, shared with batch_consolidate.hip; every
// buffer is a DevBuf / PinnedBuf, freed with the batch.  This unit holds what
// is the Solve batch's own: eligibility, the groups, the run loop, the gather
// and its decode.
//
// The problems are encoded on up to 16 host threads and uploaded one after
// another; the DevProblem structs of the batch-eligible slots are then copied
// into one device array, ordered by group, and every kernel of the Solve path
// reads its problem from that array (batch_kernels.hip, ffd_wave_batch_r.hip).
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
//  fetch_all every slot's result after one device pass: two launches
//            (batch_fetch.hip: sizes, copy) pack the batched slots' records
//            into one staging buffer (batch_fetch_layout.hpp), which comes
//            back in one transfer (two the first time after a prepare); each
//            slot is then checked and decoded by decode_result, the code the
//            per-slot fetch ends in too, on up to 16 host threads.
#include <tuple>

#include "batch_common.hpp"
#include "batch_fetch_layout.hpp"

namespace gsc {

using BatchSlot = SlotCore;  // fallback: solved through gs_run

struct Batch : BatchBase<BatchSlot> {
  bool dirty = true;  // the device array is out of date (a prepare, or a slot turned fallback)
  struct Group {
    uint32_t R, topo, wide, lp;
    uint32_t first = 0, count = 0;  // range of the device array
    uint32_t lds = 0, max_slots = 0, trunc_lds = 0;
    uint64_t max_cursors = 0, max_pairs = 0;
  };
  std::vector<Group> groups;
  std::vector<gsd::DevProblem> host;  // the device array's host image
  const gsd::DevProblem* problems() const { return (const gsd::DevProblem*)dev.data(); }
  // gs_batch_fetch_all: the payload bytes the last fetch_all of this batch found
  // (a run on the same upload finds the same): the next one's first transfer
  // carries as many
  uint64_t fetch_hint = 0;
  double fetch_gather_ms = 0, fetch_decode_ms = 0;  // the last fetch_all's device pass and decode (wall clock)
};

namespace {

constexpr uint32_t kLaunchesPerGroup = 5;

bool eligible(const gs_ctx* parent, const BatchSlot& s) {
  if (s.status != GS_OK || s.fallback) return false;
  if (parent->cfg_flags & (GS_CFG_BLOCK_SOLVE | GS_CFG_CLAIMS_HBM)) return false;
  const gs_ctx* c = s.c;
  return c->wave && !c->ch && c->dp.R >= 1 && c->dp.R <= 8 && gsd::wave_lds_bytes(c->dp, false) <= gsk_ffdw_batch_dyn_lds_max();
}

void copy_to_device(gs_ctx* c, Batch& b, size_t n) {
  b.dev.reserve(n * sizeof(gsd::DevProblem));
  if (n) {
    HIPCHK(hipMemcpyAsync(b.dev.data(), b.host.data(), n * sizeof(gsd::DevProblem), hipMemcpyHostToDevice, c->stream));
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
    by[Key{d.R, gsd::general_variant(d) ? 1u : 0u, gsd::wide_rows(d.W) ? 1u : 0u, gsk_feas_lp(d.W)}].push_back(i);
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
      g.lds = std::max(g.lds, gsd::wave_lds_bytes(d, false));
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

// gs_batch_fetch_all's device pass: the records of every slot of the device
// array in the pinned mirror.  Two launches, and one transfer of the heads and
// as much payload as the batch's last fetch_all found.  The payload's size is
// known after the synchronisation: when there is more, as in the first call
// after a prepare, a second transfer brings the rest; when there is more than
// the staging buffer holds the copy kernel wrote nothing, the buffer grows and
// the launches repeat.  Nothing here depends on how many slots there are.
struct Gathered {
  const gsbf::FetchHead* heads = nullptr;  // [order.size()]
  const char* payload = nullptr;
  uint64_t total = 0;  // payload bytes: all of them are in the mirror
};
constexpr uint64_t kFetchMinPayload = 1u << 20;

Gathered gather_all(gs_ctx* c, Batch& b, gs_batch_fetch_stats& fs) {
  const uint32_t ng = (uint32_t)b.order.size();
  const uint64_t base = gsbf::payload_base(ng);
  uint64_t worst = 0;
  uint32_t max_pods = 0;
  for (const gsd::DevProblem& d : b.host) {
    worst += gsbf::worst_bytes(gsbf::FetchBounds{d.P, d.claim_cap});
    max_pods = std::max(max_pods, d.P);
  }
  // (the mirror grows to what a call transfers; reserve_keep's `keep` bytes of it survive)
  b.fetch_hint = std::min(b.fetch_hint, worst);
  b.g_dev.reserve(base + std::max(b.fetch_hint, std::min(worst, kFetchMinPayload)));
  float dev_ms = 0;
  uint64_t cap = 0;  // payload bytes the staging buffer holds
  auto launch = [&](uint64_t bytes) {
    cap = (b.g_dev.capacity() - base) & ~(uint64_t)15u;
    HIPCHK(hipEventRecord(c->ev[6], c->stream));
    HIPCHK(gsk_fetch_gather_batch(b.problems(), ng, max_pods, b.g_dev.data(), cap, c->stream));
    HIPCHK(hipEventRecord(c->ev[7], c->stream));
    HIPCHK(hipMemcpyAsync(b.g_host.data(), b.g_dev.data(), bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    dev_ms += ms;
    fs.n_launches += 2;
    fs.n_copies++;
    fs.bytes += bytes;
    const gsbf::FetchTop top = *(const gsbf::FetchTop*)b.g_host.data();
    if (top.n != ng || top.total > worst || (top.total & 15u)) throw HipError{"gs_batch_fetch_all: corrupt gather total"};
    return top.total;
  };
  const uint64_t first = base + b.fetch_hint;
  b.g_host.reserve_keep(first, 0);
  uint64_t total = launch(first);
  if (total > cap) {
    // the copy kernel wrote nothing: a buffer that holds the total, the launches again, everything in one transfer
    b.g_dev.reserve(base + total);
    b.g_host.reserve_keep(base + total, 0);
    if (launch(base + total) != total) throw HipError{"gs_batch_fetch_all: the gather total changed between two passes"};
  } else if (total > b.fetch_hint) {
    const uint64_t rest = total - b.fetch_hint;
    b.g_host.reserve_keep(base + total, first);
    HIPCHK(hipMemcpyAsync((char*)b.g_host.data() + first, (const char*)b.g_dev.data() + first, rest, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    fs.n_copies++;
    fs.bytes += rest;
  }
  b.fetch_hint = total;
  fs.device_ms = dev_ms;
  Gathered g;
  g.heads = (const gsbf::FetchHead*)((const char*)b.g_host.data() + gsbf::kTopBytes);
  g.payload = (const char*)b.g_host.data() + base;
  g.total = total;
  return g;
}

// gs_fetch's status messages and counters for a gathered slot (h: its head,
// pay: its payload in the mirror)
gs_status decode_gathered(gs_ctx* c, const gsbf::FetchHead& h, const char* pay, gs_result* out) {
  const auto& e = c->enc;
  if (h.status != 0) return solve_status_error(c, h.status);
  const gsbf::FetchRegions r = gsbf::regions(h.n_log, h.n_claims, h.qlen);
  const SolveRecords rec{(const gsd::LogRec*)(pay + r.log),
                         h.n_log,
                         (const gsd::ClaimRec*)(pay + r.rec),
                         (const uint32_t*)(pay + r.its),
                         (const uint32_t*)(pay + r.nits),
                         h.n_claims,
                         (const uint32_t*)(pay + r.unplaced),
                         h.qlen,
                         nullptr,
                         e.node_order.data()};
  const gs_status ds = decode_result(c, rec, out);
  if (ds != GS_OK) return ds;
  c->ctrl.status = h.status;
  c->ctrl.n_claims = h.n_claims;
  c->ctrl.n_log = h.n_log;
  c->ctrl.qhead = h.qhead;
  c->ctrl.qlen = h.qlen;
  fill_solve_stats(c, h, out);
  return GS_OK;
}

}  // namespace

void batch_destroy(gs_ctx* c) {
  delete c->batch;  // its slots and buffers with it
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
  b.fetch_hint = 0;
  b.fstats = gs_batch_fetch_stats{};
  b.fetch_gather_ms = b.fetch_decode_ms = 0;
  b.ensure_slots(c, n);
  // encode on up to 16 host threads (the encoder's own loops share its pool)
  parallel_for(n, kEncodeThreads, [&](uint32_t i) {
    BatchSlot& s = b.slots[i];
    gs_ctx* sc = s.c;
    sc->prepared = sc->ran = false;
    sc->cons_ready = false;
    sc->err.clear();
    s.fallback = false;
    if (!problems[i]) {
      s.status = fail(sc, GS_E_INVALID, "NULL problem");
      return;
    }
    const auto te = Clock::now();
    gsh::Err er = gsh::encode(problems[i], sc->enc);
    sc->t_encode = ms_since(te);
    if (er.code == GS_OK) er = capacity_check(sc->enc);
    s.status = er.code == GS_OK ? GS_OK : fail(sc, er.code, er.msg);
    sc->n_nodepools = problems[i]->n_nodepools;
  });
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
    HIPCHK(gsk_queue_records_batch(b.problems(), (uint32_t)all.size(), max_pods, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } catch (const HipError& e) {
    b.copy_status(status, n);
    return fail(c, GS_E_HIP, e.msg);
  }
  b.copy_status(status, n);
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
        const gsd::DevProblem* ds = b.problems() + g.first;
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

gs_status gs_batch_fetch_all(gs_ctx* c, gs_result* out, gs_status* status) {
  if (!c || !c->batch || !c->batch->prepared) return GS_E_INVALID;
  Batch& b = *c->batch;
  if (b.n && (!out || !status)) return fail(c, GS_E_INVALID, "gs_batch_fetch_all: NULL out or status");
  if (!b.ran) return fail(c, GS_E_INVALID, "gs_batch_fetch_all: the batch has not run");
  const auto t0 = Clock::now();
  gs_batch_fetch_stats fs{};
  fs.n_slots = b.n;
  b.fetch_gather_ms = b.fetch_decode_ms = 0;
  b.copy_status(status, b.n);
  if (b.n) std::memset(out, 0, (size_t)b.n * sizeof(*out));
  // the device array's slots that are still the batched run's (one that turned
  // fallback stays in the array until the next run and is fetched alone)
  std::vector<uint32_t> pos;  // positions to decode
  for (uint32_t p = 0; p < b.order.size(); p++)
    if (!b.slots[b.order[p]].fallback) pos.push_back(p);
  if (!pos.empty()) {
    Gathered g;
    try {
      HIPCHK(hipSetDevice(c->device));
      g = gather_all(c, b, fs);
    } catch (const HipError& e) {
      return fail(c, GS_E_HIP, e.msg);
    }
    b.fetch_gather_ms = ms_since(t0);
    const auto td = Clock::now();
    const uint32_t ng = (uint32_t)b.order.size();
    std::vector<gsbf::FetchBounds> bounds(ng);
    for (uint32_t p = 0; p < ng; p++) bounds[p] = gsbf::FetchBounds{b.host[p].P, b.host[p].claim_cap};
    std::vector<uint8_t> ok(ng, 0);
    gsbf::validate(g.heads, bounds.data(), ng, g.total, g.total, ok.data());
    // slots are independent (own encoding, own result storage, own message):
    // decode on up to the 16 threads the prepare encodes on
    parallel_for((uint32_t)pos.size(), kEncodeThreads, [&](uint32_t k) {
      const uint32_t p = pos[k], i = b.order[p];
      gs_ctx* sc = b.slots[i].c;
      if (!ok[p])
        status[i] = fail(sc, GS_E_HIP, "gs_batch_fetch_all: corrupt gathered records");
      else
        status[i] = decode_gathered(sc, g.heads[p], g.payload + g.heads[p].off, &out[i]);
    });
    for (uint32_t p : pos)
      if (status[b.order[p]] == GS_OK) fs.n_decided++;
    b.fetch_decode_ms = ms_since(td);
  }
  // the run's fallback slots: gs_fetch, as gs_batch_fetch does
  for (uint32_t i = 0; i < b.n; i++) {
    BatchSlot& s = b.slots[i];
    if (s.status != GS_OK || !s.fallback) continue;
    status[i] = gs_fetch(s.c, &out[i]);
    if (status[i] != GS_OK) {
      std::memset(&out[i], 0, sizeof(out[i]));
      fs.n_copies++;
      fs.bytes += sizeof(gsd::Ctrl);
      continue;
    }
    const gsd::Ctrl& k = s.c->ctrl;
    const uint32_t P = s.c->enc.P;
    fs.n_copies += 1u + (k.n_log ? 1u : 0u) + (k.n_claims ? 3u : 0u) + (P ? 1u : 0u);
    fs.bytes += sizeof(gsd::Ctrl) + (uint64_t)k.n_log * sizeof(gsd::LogRec) +
                (uint64_t)k.n_claims * (sizeof(gsd::ClaimRec) + 61 * sizeof(uint32_t)) + (uint64_t)P * sizeof(uint32_t);
    fs.n_per_slot++;
  }
  fs.wall_ms = ms_since(t0);
  for (uint32_t i = 0; i < b.n; i++) {
    if (status[i] != GS_OK) {
      std::memset(&out[i], 0, sizeof(out[i]));
      continue;
    }
    gs_ctx* sc = b.slots[i].c;
    sc->t_fetch = fs.wall_ms;
    out[i].t_fetch_ms = sc->t_fetch;
    out[i].t_total_ms = sc->t_encode + sc->t_upload + sc->t_feas + sc->t_ffd + sc->t_trunc + sc->t_fetch;
  }
  b.fstats = fs;
  return GS_OK;
}

gs_status gs_batch_last_fetch(const gs_ctx* c, gs_batch_fetch_stats* out) {
  return batch_last_fetch(c ? c->batch : nullptr, out);
}

// diagnostic (not in the public header): the last gs_batch_fetch_all's wall
// clock up to the end of the device pass (out[0]) and of the decode (out[1]), ms
gs_status gs_debug_batch_fetch_ms(const gs_ctx* c, double out[2]) {
  if (!c || !out || !c->batch) return GS_E_INVALID;
  out[0] = c->batch->fetch_gather_ms;
  out[1] = c->batch->fetch_decode_ms;
  return GS_OK;
}

size_t gs_batch_error(const gs_ctx* c, uint32_t i, char* buf, size_t len) {
  return batch_error(c ? c->batch : nullptr, i, buf, len);
}

gs_status gs_batch_last_run(const gs_ctx* c, gs_batch_stats* out) {
  return batch_last_run(c ? c->batch : nullptr, out);
}

}  // extern "C"
