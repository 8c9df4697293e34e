// ctx.hpp — gs_ctx (one device context of libgpusched.so) and the host
// helpers shared by the Solve (capi.cpp) and consolidation (consolidate.cpp)
// entry points.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <map>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include/gpusched.h"
#include "encode.hpp"
#include "growbuf.hpp"
#include "kernel_api.hpp"
#include "layout.hpp"

namespace gsc {

constexpr uint32_t kMaxClaimsLds = 8192;  // LDS: 4x u16 slack + room, ord/sc/scratch u16, tmpl u8, thresholds
constexpr uint32_t kLdsBytes = 160 * 1024; // gfx950 LDS per workgroup
// the single-wave Solve (ffd_wave.hip) keeps 17 B of slack codes per existing
// node in LDS (layout.hpp wave_node_lds_bytes) beside the NodeClaims; larger
// clusters run the block kernel (ffd.hip)
constexpr uint32_t kWaveSolveMaxNodes = 6144;

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

struct HipError {
  std::string msg;
};
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) throw HipError{std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)

// the library's two kinds of grow-only buffer (growbuf.hpp): device memory and
// pinned host memory.  A member of one of these types is freed with its owner.
struct DevMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    return p;
  }
  static void free(void* p) { HIPCHK(hipFree(p)); }
};
struct PinnedMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    return p;
  }
  static void free(void* p) { HIPCHK(hipHostFree(p)); }
};
using DevBuf = GrowBuf<DevMem>;
using PinnedBuf = GrowBuf<PinnedMem>;

// one disruption candidate: <U> Candidate.instanceType / capacityType and
// getCandidatePrices' c.instanceType.Offerings.Compatible(labels).Cheapest()
struct CandInfo {
  bool priced = false;
  double price = 0;
  std::string it_name;
  bool spot = false;
};
struct CandTable {
  std::unordered_map<uint32_t, CandInfo> node;  // candidate node index -> info
  std::vector<std::string> it_name;              // catalog index -> instance-type name
  // NodePool minValues (<U> SatisfiesMinValues in
  // RemoveInstanceTypeOptionsByPriceAndMinValues): per NodePool the (key,
  // minimum) pairs, per instance type its values of those keys
  std::vector<std::vector<std::pair<std::string, int64_t>>> np_mv;
  std::vector<std::map<std::string, std::vector<std::string>>> it_vals;
};
bool mv_satisfied(const CandTable& t, uint32_t nodepool, const uint32_t* its, size_t n);

// The simulations of one gs_consolidate call (device-side layout: layout.hpp
// DevProblem consolidation fields).
struct SimPlan {
  std::vector<std::vector<uint32_t>> sets;  // candidate node indices (gs_problem order) per simulation
  std::vector<uint32_t> evaluated;          // simulations of this shard, in order
  std::vector<uint32_t> pod_off, pods;      // per evaluated simulation: pod ids in queue order
  std::vector<uint32_t> cand_off, cands;    // per evaluated simulation: device node positions removed
  uint32_t max_pods = 0, ov_cap = 0, blocks = 0, nt = 256;
  bool sim_lds = false;                     // per-simulation queue arrays and add log in LDS
  std::vector<uint64_t> known;              // per evaluated simulation: zone domains known without its candidates
  uint32_t multi_max = 0;                   // MULTI: firstNConsolidationOption's max
};

struct Batch;  // batch.cpp: the slots of gs_batch_*
void batch_destroy(gs_ctx* c);
struct ConsBatch;  // batch_consolidate.hip: the slots of gs_batch_consolidate_*
void batch_consolidate_destroy(gs_ctx* c);
void create_filter_destroy(gs_ctx* c);  // filter.hip: frees gs_ctx::cf
void rank_batch_destroy(gs_ctx* c);     // rank_batch.hip: frees gs_ctx::rank
void explain_destroy(gs_ctx* c);        // explain.hip: frees gs_ctx::explain

}  // namespace gsc
namespace gsf {
struct State;  // filter.hip: the re-filter's arena and results, its resident catalog and the runs' buffers
}
namespace gsrb {
struct State;  // rank_batch.hip: the ranking's resident catalog and the runs' buffers
}
namespace gse {
struct State;  // explain.hip: gs_explain's device buffers, staging and result storage
}

struct gs_ctx {
  int device = 0;
  uint32_t cfg_flags = 0;  // gs_config.flags
  std::vector<gs_ctx*> shards;  // gs_config.n_shards > 1: one child context per shard (multi.cpp)
  gsc::Batch* batch = nullptr;  // gs_batch_*: one child context per slot, on this context's stream and events (batch.cpp)
  gsc::ConsBatch* cons_batch = nullptr;  // gs_batch_consolidate_*: likewise (batch_consolidate.hip)
  std::vector<ncclComm_t> comms;  // GS_CFG_RCCL: one communicator rank per shard (ncclCommInitAll)
  std::string err;
  hipStream_t stream = nullptr;
  hipEvent_t ev[8] = {};
  std::vector<void*> allocs;
  gsh::Encoded enc;
  gsd::DevProblem dp{};
  bool prepared = false, ran = false;
  bool wave = false;  // the prepared Solve runs the single-wave kernel
  bool ch = false;    // ... with its claim scan state in HBM (grown past the LDS NodeClaims)
  uint32_t n_nodepools = 0;  // of the prepared problem (the caller's arrays are not kept)
  double t_encode = 0, t_upload = 0, t_feas = 0, t_ffd = 0, t_trunc = 0, t_fetch = 0, t_run_wall = 0;
  // result storage
  std::vector<uint32_t> claim_nodepool, claim_pod_offsets, claim_pods, claim_it_offsets, claim_its;
  std::vector<std::string> req_text;
  std::vector<const char*> req_ptrs;
  std::vector<int64_t> claim_requests;
  std::vector<uint32_t> node_pod_offsets, node_pods, error_pods;
  std::vector<uint64_t> f_rows;
  std::vector<int32_t> f_cheapest;
  std::vector<uint32_t> f_nfo;
  std::vector<uint64_t> f_key;
  std::vector<uint32_t> f_var_of_pod, f_tmpl_np;
  gsd::Ctrl ctrl{};
  // consolidation: the combined problem (pending ++ bound pods), the plan,
  // the input copy (rerun) and result storage
  std::vector<gs_pod> cons_pods;
  gs_problem cons_problem{};
  gs_consolidation cons_in{};
  std::vector<uint32_t> cons_cands;
  std::vector<gs_range> cons_sets;
  uint32_t n_pending = 0;
  gsc::SimPlan sims;
  gsc::CandTable cand_table;
  std::vector<gs_command> commands;
  std::vector<uint32_t> cmd_options;
  std::vector<double> cmd_prices;
  std::vector<uint32_t> multi_opts;
  bool cons_ready = false;
  // the decided table's policy outcome and counter sums (cons_fill_result)
  int32_t cons_chosen = -1;
  uint64_t cons_checks = 0, cons_node_evals = 0, cons_node_prefix = 0, cons_pops = 0;
  // pinned per-simulation result staging (allocated with the plan)
  gsd::SimCtrl* h_ctrl = nullptr;
  std::vector<gsd::Ctrl> h_blk;  // the simulation workgroups' counter sums
  gsd::ClaimRec* h_hdr = nullptr;
  uint32_t* h_its = nullptr;
  uint32_t* h_nits = nullptr;
  // ... and the same as the records the decision reads (cons_decide_records)
  std::vector<gsd::SimOut> h_rec;
  std::vector<gsd::OptPair> h_pairs;
  double t_sim = 0;
  // gs_consolidation_results: the re-run simulation's per-NodeClaim top 60
  // (device; one slot per pod of the largest simulation)
  uint32_t* res_its = nullptr;
  uint32_t* res_nits = nullptr;
  uint32_t* res_drop = nullptr;

  gsf::State* cf = nullptr;  // gs_create_filter and gs_create_filter_prepare / _run (filter.hip)
  gsrb::State* rank = nullptr;  // gs_rank_prepare / _run (rank_batch.hip)
  gse::State* explain = nullptr;  // gs_explain (explain.hip)
  // gs_build_catalog result storage
  std::vector<std::string> cat_strs, cat_reasons;
  std::vector<const char*> cat_ptrs, cat_reason_ptrs;
  std::vector<uint32_t> cat_vals, cat_skipped;
  std::vector<gs_requirement> cat_reqs;
  std::vector<gs_quantity> cat_qty;
  std::vector<gs_offering> cat_offs;
  std::vector<gs_instance_type> cat_its;

  std::vector<void*> host_allocs;  // pinned staging buffers (consolidation results)
  void free_all() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    for (void* p : host_allocs) (void)hipHostFree(p);
    host_allocs.clear();
  }
  // Device buffers of one prepared problem come from ONE allocation (an arena
  // of 256-B aligned sub-buffers): large pages, few TLB entries for the
  // single-workgroup FFD kernel's gathers.  plan() records, commit() places.
  // The arena and a pinned staging image of the uploaded buffers persist
  // across prepares and only grow: commit() lays the
  // uploaded buffers out first, copies their host arrays once into the
  // pinned image and issues one H2D copy, without re-hipMalloc per prepare.
  struct Planned {
    void** dst;
    size_t bytes;
    const void* src;  // uploaded host bytes (nullptr: device-only buffer)
    bool zero;
  };
  std::vector<Planned> plan;
  std::vector<std::shared_ptr<void>> keep;  // host arrays built for one upload (live until commit)
  size_t plan_bytes = 0;
  size_t ov_hn_bytes = 0;  // the simulation overlay cells (cleared when the stamp prefix wraps)
  size_t hc_bytes = 0;     // simulations: the NodeClaim hostname-count rows (zero at rest)
  gsc::DevBuf arena;
  gsc::PinnedBuf stage;
  // memory only (with the two members above): a batch slot borrows its
  // parent's stream and events, which gs_destroy destroys for their owner
  ~gs_ctx() { free_all(); }
  template <class P>
  void alloc(P*& dst, size_t n) {
    const size_t b = std::max<size_t>(n, 1) * sizeof(P);
    plan.push_back(Planned{(void**)&dst, b, nullptr, false});
    plan_bytes += (b + 255) & ~(size_t)255;
  }
  template <class P>
  void alloc_zero(P*& dst, size_t n) {
    alloc(dst, n);
    plan.back().zero = true;
  }
  // v must live until commit(): the encoder's arrays (c->enc) or, through
  // the rvalue overload, a temporary kept here
  template <class P, class T>
  void upload(P*& dst, const std::vector<T>& v) {
    static_assert(sizeof(P) == sizeof(T), "upload type");
    alloc(dst, v.size());
    if (!v.empty()) plan.back().src = v.data();
  }
  template <class P, class T>
  void upload(P*& dst, std::vector<T>&& v) {
    auto h = std::make_shared<std::vector<T>>(std::move(v));
    keep.push_back(h);
    upload(dst, *h);
  }
  double t_stage_ms = 0, t_h2d_ms = 0;  // commit's split: host copy into the pinned image, H2D + memsets
  void commit();
};

namespace gsc {

gs_status fail(gs_ctx* c, gs_status s, const std::string& m);
gs_status prepare_one(gs_ctx* c, const gs_problem* p);  // gs_prepare on one device
gs_status prepare_from(gs_ctx* c, const gs_ctx* src);    // upload another context's encoding (shards)
void launch_feas(gs_ctx* c, uint32_t apply_limits, uint32_t w_lo = 0, uint32_t w_hi = ~0u, bool mv_rows = true);
// the static matrix of words [wb, we) on every shard, merged into the parent's device buffers
gs_status sharded_compute(gs_ctx* c, uint32_t wb, uint32_t we, double* kernel_ms, double* merge_ms);
// multi.cpp: contexts with shards
gs_status sharded_prepare(gs_ctx* c, const gs_problem* p);
gs_status sharded_consolidate(gs_ctx* c, const gs_consolidation* in, gs_consolidation_result* out);
CandTable build_cand_table(const gs_problem* p, const uint32_t* cands, uint32_t n);
int32_t choose_commands(const CandTable& t, const gs_consolidation* in, const gs_command* commands,
                        const uint32_t* options, const double* prices, std::vector<uint32_t>* multi);
gsh::Err capacity_check(const gsh::Encoded& e);
// One Solve's device records, copied to the host: the add log, the NodeClaim
// headers with their OrderByPrice top 60 ([n_claims][60] / [n_claims]), the
// pods still queued at the end, and the maps from the records' pod ids
// (nullptr: they are the caller's already) and node positions to the caller's
// indices.
struct SolveRecords {
  const gsd::LogRec* log;
  uint32_t n_log;
  const gsd::ClaimRec* hdr;
  const uint32_t* its;
  const uint32_t* nits;
  uint32_t n_claims;
  const uint32_t* unplaced;
  uint32_t n_unplaced;
  const uint32_t* pod_index;
  const uint32_t* node_index;
};
gs_status decode_result(gs_ctx* c, const SolveRecords& r, gs_result* out);
// The fetch epilogue gs_fetch and gs_batch_fetch_all (batch.cpp) share:
// the failure a Solve's non-zero control status stands for, and the counters,
// phase timers, sizes and stage times of a fetched Solve.  H: gsd::Ctrl or
// gsbf::FetchHead (the same field names).
gs_status solve_status_error(gs_ctx* c, uint32_t status);
template <class H>
void fill_solve_stats(const gs_ctx* c, const H& h, gs_result* out);  // capi.cpp instantiates both
// multi.cpp: gs_consolidation_results on the shard that evaluated `sim`
gs_status sharded_results(gs_ctx* c, uint32_t sim, gs_result* out);
uint32_t trunc_lds_bytes(uint32_t N);
// encode output -> device arena; `sims` non-null: consolidation arenas
// (records: gather the Solve's first-pass queue records after the upload;
// false for a batch slot, whose batch gathers every slot's in one launch)
void upload_problem(gs_ctx* c, const SimPlan* sims, bool records = true);

// consolidate.cpp: gs_consolidate in the steps a batch drives per slot
// (batch_consolidate.hip): check, take the input and encode, plan, upload,
// launch, fetch and decide.
// threads per simulation workgroup for n simulations on a device of `cus`
// CUs: many simulations take the narrow shape (throughput), few the wide one
// (each simulation's latency) -- ffd_block.hpp FB_SIM / FB_SIM_NARROW
inline uint32_t cons_sim_threads(size_t n_sims, int cus) { return n_sims >= 4 * (size_t)std::max(cus, 1) ? 128u : 256u; }
// what a batch gives a slot's plan instead of the whole device
struct SimBudget {
  uint32_t nt;          // the batch's shape
  uint64_t group_sims;  // simulations of the slot's group (the slots launched together)
};
gs_status cons_check_input(const gs_consolidation* in, std::string* err);
gs_status cons_take_input(gs_ctx* c, const gs_consolidation* in);
gs_status cons_plan_sets(gs_ctx* c, std::string* err);
gs_status cons_plan_grid(gs_ctx* c, const SimBudget* budget, std::string* err);
gs_status cons_upload(gs_ctx* c);
gs_status cons_launch(gs_ctx* c);
gs_status cons_fetch_decide(gs_ctx* c, gs_consolidation_result* out);
// the decision alone, from packed records: rec[k] per evaluated simulation, its
// options at opts[rec[k].opt_off ...], the slot's counter sums
gs_status cons_decide_records(gs_ctx* c, const gsd::SimOut* rec, const gsd::OptPair* opts, const gsd::SlotOut& sums);
void cons_fill_result(const gs_ctx* c, gs_consolidation_result* out);
gs_status cons_sim_results(gs_ctx* c, uint32_t sim, gs_result* out);
void reset_sim_counts(gs_ctx* c);
void next_overlay_epoch(gs_ctx* c);

}  // namespace gsc

inline void gs_ctx::commit() {
  using gsc::HipError;
  // uploaded buffers first (one contiguous image), then zeroed, then the rest
  size_t off_up = 0, off_zero = 0, off_rest = 0;
  for (auto& q : plan)
    if (q.src) off_up += gsc::up256(q.bytes);
    else if (q.zero) off_zero += gsc::up256(q.bytes);
    else off_rest += gsc::up256(q.bytes);
  const size_t n_up = off_up, n_zero = off_zero, total = std::max<size_t>(n_up + n_zero + off_rest, 256);
  arena.reserve(total);  // with headroom: a slightly larger problem reuses it
  stage.reserve(n_up);
  char* base = (char*)arena.data();
  std::vector<gsh::HostCopy> copies;
  size_t a = 0, z = n_up, r = n_up + n_zero;
  for (auto& q : plan) {
    if (q.src) {
      *q.dst = base + a;
      copies.push_back({q.src, a, q.bytes});
      a += gsc::up256(q.bytes);
    } else if (q.zero) {
      *q.dst = base + z;
      z += gsc::up256(q.bytes);
    } else {
      *q.dst = base + r;
      r += gsc::up256(q.bytes);
    }
  }
  const auto t0 = gsc::Clock::now();
  gsh::host_copy_parallel(stage.data(), copies.data(), copies.size());
  t_stage_ms = gsc::ms_since(t0);
  const auto t1 = gsc::Clock::now();
  if (n_up) HIPCHK(hipMemcpyAsync(base, stage.data(), n_up, hipMemcpyHostToDevice, stream));
  if (n_zero) HIPCHK(hipMemsetAsync(base + n_up, 0, n_zero, stream));
  HIPCHK(hipStreamSynchronize(stream));
  t_h2d_ms = gsc::ms_since(t1);
  static const bool prof = std::getenv("GS_ENCODE_PROFILE") != nullptr;
  if (prof)
    std::fprintf(stderr, "upload.stage %.3f ms  upload.h2d %.3f ms  (%zu B uploaded, %zu B zeroed, %zu B total)\n",
                 t_stage_ms, t_h2d_ms, n_up, n_zero, total);
  plan.clear();
  keep.clear();
  plan_bytes = 0;
}
