// batch_kernels.hip — the Solve path's grid kernels over a device array of
// independent problems (gs_batch_*).  The kernels are the single-problem
// ones, compiled here in their batched form (kernel_problem.hpp): the problem
// is element blockIdx.y of `ds`, gridDim.x is sized for the largest problem of
// the launch, and a block or wave past its own problem's extent returns
// before any barrier or LDS use (each kernel's own bound check on V x T, P or
// the NodeClaim count, which is uniform over the wave or the block where the
// kernel has a barrier).  The index is uniform over the workgroup, so a
// problem's fields arrive by scalar loads as kernel arguments do.  The
// batched single-wave Solve is in ffd_wave_batch_r.hip, the batched simulation
// kernel (gs_batch_consolidate_*) in ffd_sim_batch_r.hip.
#define GS_BATCH_KERNELS 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devutil.hpp"
#include "ffd_common.hpp"
#include "kernel_api.hpp"
#include "layout.hpp"

using namespace gsd;

#include "solve_kernels.hpp"
#include "queue_kernels.hpp"
#include "init_kernel.hpp"

// ------------------------------------------------------------ host launchers
extern "C" hipError_t gsk_init_batch(uint32_t trunc_lds_bytes) {
  return hipFuncSetAttribute((const void*)trunc_kernel_batch, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)trunc_lds_bytes);
}

// the lane-pair width gsk_feas (kernels.hip) picks for rows of W words
extern "C" uint32_t gsk_feas_lp(uint32_t W) {
#ifndef GS_K1_LPMAX
#define GS_K1_LPMAX 16
#endif
  if (GS_K1_LPMAX < 64 && W > GS_K1_LPMAX && W <= 32 && W * (64 / GS_K1_LPMAX) <= 256) W = GS_K1_LPMAX;
  uint32_t lp = 1;
  while (lp < W && lp < 64) lp <<= 1;
  return lp;
}

template <uint32_t LP>
static void launch_feas_batch_lp(const DevProblem* ds, uint32_t n, uint64_t max_pairs, hipStream_t s) {
  const uint64_t per_block = (BLOCK / 64) * (64 / LP);
  const uint32_t blocks = (uint32_t)((max_pairs + per_block - 1) / per_block);
  hipLaunchKernelGGL(feas_kernel_batch<LP>, dim3(blocks ? blocks : 1, n), dim3(BLOCK), 0, s, ds, 0u, 0u, ~0u);
}

// K1/K2 of n problems that share the lane-pair width lp, as the Solve runs them
// (static_mode 0, every instance-type word): two launches.
// max_cursors / max_pairs: the largest V x T x R and V x T among them.
extern "C" hipError_t gsk_feas_batch(const DevProblem* ds, uint32_t n, uint32_t lp, uint64_t max_cursors,
                                     uint64_t max_pairs, hipStream_t s) {
  if (!n || n > 65535) return hipErrorInvalidValue;
  const uint32_t cb = (uint32_t)((max_cursors + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(feas_cursor_kernel_batch, dim3(cb ? cb : 1, n), dim3(BLOCK), 0, s, ds);
  switch (lp) {
    case 1: launch_feas_batch_lp<1>(ds, n, max_pairs, s); break;
    case 2: launch_feas_batch_lp<2>(ds, n, max_pairs, s); break;
    case 4: launch_feas_batch_lp<4>(ds, n, max_pairs, s); break;
    case 8: launch_feas_batch_lp<8>(ds, n, max_pairs, s); break;
    case 16: launch_feas_batch_lp<16>(ds, n, max_pairs, s); break;
    case 32: launch_feas_batch_lp<32>(ds, n, max_pairs, s); break;
    case 64: launch_feas_batch_lp<64>(ds, n, max_pairs, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// the state reset of n problems: one launch (the single problem's reset is 256
// blocks of grid-stride loops; a batch gives each problem 8)
extern "C" hipError_t gsk_init_state_batch(const DevProblem* ds, uint32_t n, hipStream_t s) {
  if (!n || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ffd_init_kernel_batch, dim3(8, n), dim3(256), 0, s, ds);
  return hipGetLastError();
}

// the first-pass queue records of n problems (after their uploads): one launch
extern "C" hipError_t gsk_queue_records_batch(const DevProblem* ds, uint32_t n, uint32_t max_pods, hipStream_t s) {
  if (!n || !max_pods) return hipSuccess;
  if (n > 65535) return hipErrorInvalidValue;
  const uint32_t blocks = (max_pods + 255) / 256;
  hipLaunchKernelGGL(queue_records_kernel_batch, dim3(blocks, n), dim3(256), 0, s, ds);
  return hipGetLastError();
}

// K3 of n problems: max_slots NodeClaim slots per problem, one launch
extern "C" hipError_t gsk_trunc_batch(const DevProblem* ds, uint32_t n, uint32_t max_slots, uint32_t lds_bytes,
                                      hipStream_t s) {
  if (!n || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trunc_kernel_batch, dim3(max_slots ? max_slots : 1, n), dim3(BLOCK), lds_bytes, s, ds, 0u, 0u);
  return hipGetLastError();
}

// ------------------------------------------------ the batched single-wave Solve
// The instantiations live in ffd_wave_batch_r.hip, and those of the batched
// simulation kernel in ffd_sim_batch_r.hip, one translation unit per
// (R, TOPO): each exports its family record (kernel_api.hpp).
static auto& ffdwb_families() {
#define GSK_ENTRY(r, t) GSK_RT_NAME(gsk_ffdwb, r, t)(),
  static const GskWaveBatchFamily* const table[] = {GSK_FOR_EACH_RT(GSK_ENTRY)};
#undef GSK_ENTRY
  return table;
}
static auto& ffdsb_families() {
#define GSK_ENTRY(r, t) GSK_RT_NAME(gsk_ffdsb, r, t)(),
  static const GskSimBatchFamily* const table[] = {GSK_FOR_EACH_RT(GSK_ENTRY)};
#undef GSK_ENTRY
  return table;
}
static uint32_t g_ffdwb_dyn_max = 0;

extern "C" hipError_t gsk_init_ffdw_batch(uint32_t lds_total) { return gsk_set_lds(ffdwb_families(), lds_total, &g_ffdwb_dyn_max); }

extern "C" uint32_t gsk_ffdw_batch_dyn_lds_max(void) { return g_ffdwb_dyn_max; }

// n problems of one instantiation (R resources, the general variant or not,
// wide option rows or not), one workgroup each: one launch.  lds: the largest
// dynamic LDS among them (gsk_ffdw's formula per problem).
extern "C" hipError_t gsk_ffdw_batch(const DevProblem* ds, uint32_t n, uint32_t R, uint32_t topo, uint32_t wide,
                                     uint32_t lds, hipStream_t s) {
  if (!n || lds > g_ffdwb_dyn_max) return hipErrorInvalidConfiguration;
  const GskWaveBatchFamily* f = gsk_family(ffdwb_families(), R, topo != 0);
  return f ? f->launch(ds, n, wide, lds, s) : hipErrorInvalidValue;
}

// ===================================== consolidation simulations of n problems
// (gs_batch_consolidate_*)

// What a launch of the simulation kernel needs reset, for every problem of a
// group in one launch: the work counter, and (clear_overlays: the launch's
// stamp prefix wrapped) the overlay hostname-count cells of the problem's
// blocks[y] workgroups.
extern "C" __global__ __launch_bounds__(256) void sim_begin_kernel_batch(const DevProblem* __restrict__ ds,
                                                                         const uint32_t* __restrict__ blocks,
                                                                         uint32_t clear_overlays) {
  const DevProblem& d = ds[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0) *d.sim_next = 0;
  if (!clear_overlays) return;
  const size_t cells = (size_t)blocks[blockIdx.y] * d.ov_cap * (d.TGH ? d.TGH : 1u);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) d.ov_hn[i] = 0;
}

extern "C" hipError_t gsk_sim_begin_batch(const DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t clear_overlays,
                                          hipStream_t s) {
  if (!n || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sim_begin_kernel_batch, dim3(clear_overlays ? 8 : 1, n), dim3(256), 0, s, ds, blocks, clear_overlays);
  return hipGetLastError();
}

// K3 of n problems' simulations, as gsk_trunc runs it for one: block s of a
// problem truncates simulation s's single NodeClaim; with minValues (mv) every
// NodeClaim arena slot (max_slots: the largest problem's simulated pods), then
// the per-simulation settlement.  max_sims: the largest problem's simulations.
extern "C" hipError_t gsk_trunc_sims_batch(const DevProblem* ds, uint32_t n, uint32_t mv, uint32_t max_sims,
                                           uint32_t max_slots, uint32_t lds_bytes, hipStream_t s) {
  if (!n || n > 65535) return hipErrorInvalidValue;
  if (mv) {
    hipLaunchKernelGGL(trunc_kernel_batch, dim3(max_slots ? max_slots : 1, n), dim3(BLOCK), lds_bytes, s, ds, 1u, 0u);
    hipLaunchKernelGGL(sim_fix_kernel_batch, dim3((max_sims + BLOCK - 1) / BLOCK ? (max_sims + BLOCK - 1) / BLOCK : 1, n),
                       dim3(BLOCK), 0, s, ds);
  } else {
    hipLaunchKernelGGL(trunc_kernel_batch, dim3(max_sims ? max_sims : 1, n), dim3(BLOCK), lds_bytes, s, ds, 0u, 0u);
  }
  return hipGetLastError();
}

static uint32_t g_ffdsb_dyn_max = 0;

extern "C" hipError_t gsk_init_ffd_sim_batch(uint32_t lds_total) { return gsk_set_lds(ffdsb_families(), lds_total, &g_ffdsb_dyn_max); }

extern "C" uint32_t gsk_ffd_sim_batch_dyn_lds_max(void) { return g_ffdsb_dyn_max; }

// resident workgroups per CU of the batched simulation kernel (R resources,
// the general variant or not, nt threads) at a dynamic LDS size; at least 1
extern "C" uint32_t gsk_ffd_sim_batch_blocks_per_cu(uint32_t R, uint32_t lds, uint32_t nt, uint32_t general) {
  const GskSimBatchFamily* f = gsk_family(ffdsb_families(), R, general != 0);
  const uint32_t n = f ? f->blocks_per_cu(nt, lds) : 0u;
  return n ? n : 1u;
}

// the simulations of n problems of one instantiation (R resources, the general
// variant or not, nt threads per workgroup): blocks[i] persistent workgroups
// for problem i, one launch.  lds: the largest dynamic LDS among them
// (gsk_ffd's formula per problem).
extern "C" hipError_t gsk_ffd_sim_batch(const DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t max_blocks,
                                        uint32_t R, uint32_t general, uint32_t nt, uint32_t lds, uint32_t ov_epoch,
                                        hipStream_t s) {
  if (!n || n > 65535 || !max_blocks) return hipErrorInvalidValue;
  if (lds > g_ffdsb_dyn_max) return hipErrorInvalidConfiguration;
  const GskSimBatchFamily* f = gsk_family(ffdsb_families(), R, general != 0);
  return f ? f->launch(ds, blocks, n, max_blocks, nt, lds, ov_epoch, s) : hipErrorInvalidValue;
}

// ===================== every slot's outcome in one pass (gs_batch_consolidate_fetch_all)
// Two kernels per group over the array the run used, writing into one
// batch-wide staging buffer: SlotOut per slot, SimOut per evaluated simulation
// (slot y's simulation k at recs[sim_base[y] + k]: the host knows every slot's
// simulation count from its plan), and the options of the single-NodeClaim
// simulations compacted behind one another.
//
// Option offsets: the settle kernel scans the slot's option counts in
// simulation order (SimOut::opt_off, relative to the slot) and takes the slot's
// share of the option region with one atomic add on the batch's cursor, which
// the host clears before the first group (SlotOut::opt_base).  Slots therefore
// lie in the region in arrival order; each slot's options are in simulation
// order.  The cursor's final value is the number of options to transfer.

// One workgroup per slot: the outcome records and the counter sums.
extern "C" __global__ __launch_bounds__(256) void cons_settle_kernel_batch(const DevProblem* __restrict__ ds,
                                                                           const uint32_t* __restrict__ blocks,
                                                                           const uint32_t* __restrict__ sim_base,
                                                                           SlotOut* __restrict__ slots,
                                                                           SimOut* __restrict__ recs,
                                                                           uint32_t* __restrict__ cursor) {
  const DevProblem& d = ds[blockIdx.y];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t NS = d.n_sims;
  SimOut* out = recs + sim_base[blockIdx.y];
  __shared__ uint32_t s_wave[4];
  __shared__ unsigned long long s_sum[3];
  if (tid < 3) s_sum[tid] = 0;
  uint32_t run = 0;  // options of the simulations before this chunk (uniform)
  for (uint32_t k0 = 0; k0 < NS; k0 += 256) {
    const uint32_t k = k0 + tid;
    SimOut o{};
    if (k < NS) {
      const SimCtrl ct = d.sim_ctrl[k];
      o.status = ct.status;
      o.n_claims = ct.n_claims;
      o.failed = ct.failed;
      if (ct.status == 0 && ct.failed == 0 && ct.n_claims == 1) {
        const ClaimRec& h = d.sim_hdr[k];
        o.tmpl = h.tmpl;
        o.ctb = h.ctb;
        o.zflags = h.zflags;
        o.zfull = h.zfull;
        o.zm = h.zm;
        o.cm = h.cm;
        const uint32_t n = d.c_nits[k];
        o.n_opt = n < SIM_OPTS_MAX ? n : SIM_OPTS_MAX;
      }
    }
    // exclusive scan of n_opt over the chunk: within the wave, then over the 4 waves
    uint32_t incl = o.n_opt;
    for (uint32_t s = 1; s < 64; s <<= 1) {
      const uint32_t up = __shfl_up(incl, s, 64);
      if (lane >= s) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < 4; w++) {
      before += w < wave ? s_wave[w] : 0u;
      total += s_wave[w];
    }
    __syncthreads();  // s_wave is rewritten by the next chunk
    if (k < NS) {
      o.opt_off = run + before + incl - o.n_opt;
      out[k] = o;
    }
    run += total;
  }
  // the simulation workgroups' counters
  unsigned long long ne = 0, np = 0, pp = 0;
  for (uint32_t b = tid; b < blocks[blockIdx.y]; b += 256) {
    const Ctrl& c = d.sim_blk[b];
    ne += c.node_evals;
    np += c.node_prefix;
    pp += c.pops;
  }
  __syncthreads();  // s_sum cleared
  if (ne) atomicAdd(&s_sum[0], ne);
  if (np) atomicAdd(&s_sum[1], np);
  if (pp) atomicAdd(&s_sum[2], pp);
  __syncthreads();
  if (tid == 0) {
    SlotOut so;
    so.node_evals = s_sum[0];
    so.node_prefix = s_sum[1];
    so.pops = s_sum[2];
    so.n_opt = run;
    so.opt_base = run ? atomicAdd(cursor, run) : 0u;
    slots[blockIdx.y] = so;
  }
}

// One wave per evaluated simulation, one lane per option: the instance type
// and the price rank of its cheapest available offering on the NodeClaim's grid
// (cons_fetch_decide's inner loop).  gridDim.x is sized for the group's largest
// slot; a wave past its own slot's simulations, or whose simulation has no
// option list, returns (no barrier, no LDS).
extern "C" __global__ __launch_bounds__(256) void cons_options_kernel_batch(const DevProblem* __restrict__ ds,
                                                                            const uint32_t* __restrict__ sim_base,
                                                                            const SlotOut* __restrict__ slots,
                                                                            const SimOut* __restrict__ recs,
                                                                            OptPair* __restrict__ opts) {
  const DevProblem& d = ds[blockIdx.y];
  const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (k >= d.n_sims) return;
  const SimOut& o = recs[sim_base[blockIdx.y] + k];
  if (lane >= o.n_opt) return;
  const uint32_t it = d.c_its[(size_t)k * 60 + lane];
  OptPair p;
  p.it = it;
  p.minp = it < d.N ? option_min_rank(d.it_pair, d.it_prank, it, pair_grid(o.zm, o.cm, d.Z, d.C)) : NONE;
  opts[(size_t)slots[blockIdx.y].opt_base + o.opt_off + lane] = p;
}

// n slots of one group (ds, blocks, sim_base and slots point at the group's
// first): two launches.  max_sims: the largest slot's simulations.
extern "C" hipError_t gsk_cons_gather_batch(const DevProblem* ds, const uint32_t* blocks, const uint32_t* sim_base,
                                            uint32_t n, uint32_t max_sims, SlotOut* slots, SimOut* recs, OptPair* opts,
                                            uint32_t* cursor, hipStream_t s) {
  if (!n || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cons_settle_kernel_batch, dim3(1, n), dim3(256), 0, s, ds, blocks, sim_base, slots, recs, cursor);
  hipLaunchKernelGGL(cons_options_kernel_batch, dim3(max_sims ? (max_sims + 3) / 4 : 1, n), dim3(256), 0, s, ds, sim_base,
                     (const SlotOut*)slots, (const SimOut*)recs, opts);
  return hipGetLastError();
}
