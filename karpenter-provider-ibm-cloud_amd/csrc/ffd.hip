// ffd.hip — K4: the <U> Scheduler.Solve queue loop (first-fit decreasing over
// existing/in-flight/new NodeClaims) as ONE persistent 1024-thread workgroup.
//
// Per popped pod:
//  1. sort.Slice(newNodeClaims, len(Pods) asc) is reproduced EXACTLY (Go's
//     pdqsort_func permutes ties; which NodeClaim a pod lands on depends on
//     it).  Between two sorts at most one NodeClaim changed (one pod added,
//     or one NodeClaim appended), so the common case is resolved in O(1)
//     decisions + one parallel rotation (see DESIGN.md "sort emulation");
//     every other case runs a block-parallel restatement of pdqsort_func
//     whose partition / partitionEqual / partialInsertionSort passes are
//     ballot-prefix compactions over LDS.
//  2. in-flight NodeClaims are scored 1024 at a time in sorted order; a cheap
//     necessary test (tolerated template, per-resource slack upper bound)
//     gates the exact NodeClaim.CanAdd (free-key Compatible, instance-type
//     bitset AND, fits via per-resource threshold bitsets, offering grid);
//     the first feasible position wins (block min).
//  3. otherwise templates in weight order open a new NodeClaim from the
//     precomputed K1 row (limits applied dynamically); else Relax + requeue.
//
// The kernel and its helpers are in ffd_block.hpp (shared with the batched
// simulation units, ffd_sim_batch_r.hip); this unit instantiates the
// single-problem forms and holds their launchers.
#include "ffd_block.hpp"
#include "kernel_api.hpp"

// The six shapes of the block kernel for one resource count: the provisioning
// Solve [general] and the simulations [general][narrow] (FB_SIM or
// FB_SIM_NARROW threads per workgroup).  One record per R of the family list;
// launch, LDS attribute and occupancy all read it.
using BlockKernel = void (*)(DevProblem);
struct BlockFamily {
  uint32_t R;
  BlockKernel solve[2];
  BlockKernel sim[2][2];
};
template <uint32_t RR>
static const BlockFamily* block_family() {
  static const BlockFamily f = {RR,
                                {ffd_kernel<RR, false, FB_MAX, false>, ffd_kernel<RR, false, FB_MAX, true>},
                                {{ffd_kernel<RR, true, FB_SIM, false>, ffd_kernel<RR, true, FB_SIM_NARROW, false>},
                                 {ffd_kernel<RR, true, FB_SIM, true>, ffd_kernel<RR, true, FB_SIM_NARROW, true>}}};
  return &f;
}
static auto& ffd_families() {
#define GSK_ENTRY(r, unused) block_family<r>(),
  static const BlockFamily* const table[] = {GSK_FOR_EACH_R(GSK_ENTRY, )};
#undef GSK_ENTRY
  return table;
}
// the record of R; nullptr: R outside 1..8
static const BlockFamily* ffd_family(uint32_t R) {
  for (const BlockFamily* f : ffd_families())
    if (f->R == R) return f;
  return nullptr;
}

// every instantiation may use all LDS its static footprint leaves free
static uint32_t g_ffd_dyn_max = 0;

extern "C" hipError_t gsk_init_ffd(uint32_t lds_total) {
  hipError_t e = hipSuccess;
  for (const BlockFamily* f : ffd_families())
    for (BlockKernel fn : {f->solve[0], f->solve[1], f->sim[0][0], f->sim[0][1], f->sim[1][0], f->sim[1][1]})
      if (hipError_t x = set_max_dyn_lds((const void*)fn, lds_total, &g_ffd_dyn_max); x != hipSuccess) e = x;
  return e;
}

extern "C" uint32_t gsk_ffd_dyn_lds_max(void) { return g_ffd_dyn_max; }

// resident simulation workgroups per CU for a given dynamic LDS size
extern "C" uint32_t gsk_ffd_sim_blocks_per_cu(uint32_t R, uint32_t lds, uint32_t nt, uint32_t general) {
  int n = 0;
  const BlockFamily* f = ffd_family(R);
  const bool narrow = nt == (uint32_t)FB_SIM_NARROW;
  const hipError_t e = f ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)f->sim[general != 0][narrow],
                                                                        narrow ? FB_SIM_NARROW : FB_SIM, lds)
                         : hipErrorInvalidValue;
  return e == hipSuccess && n > 0 ? (uint32_t)n : 1u;
}

// grid: 1 workgroup (provisioning Solve) or `blocks` persistent workgroups
// draining the simulation counter (consolidation)
extern "C" hipError_t gsk_ffd(const DevProblem* d, uint32_t blocks, hipStream_t s) {
  const bool sim = d->n_sims > 0, general = general_variant(*d);
  const uint32_t lds = sim ? sim_lds_bytes(*d) : block_lds_bytes(*d);
  if (lds > g_ffd_dyn_max) return hipErrorInvalidConfiguration;
  if (sim && d->sim_nt != (uint32_t)FB_SIM && d->sim_nt != (uint32_t)FB_SIM_NARROW) return hipErrorInvalidValue;
  const BlockFamily* f = ffd_family(d->R);
  if (!f) return hipErrorInvalidValue;
  if (sim) hipLaunchKernelGGL(f->sim[general][d->sim_nt == (uint32_t)FB_SIM_NARROW], dim3(blocks), dim3(d->sim_nt), lds, s, *d);
  else hipLaunchKernelGGL(f->solve[general], dim3(1), dim3(FB_MAX), lds, s, *d);
  return hipGetLastError();
}

// the first-pass queue record kernels (shared with the batched kernels of batch_kernels.hip)
#include "queue_kernels.hpp"

extern "C" hipError_t gsk_queue_records(const DevProblem* d, hipStream_t s) {
  if (!d->P) return hipSuccess;
  hipLaunchKernelGGL(queue_records_kernel, dim3((d->P + 255) / 256), dim3(256), 0, s, *d);
  return hipGetLastError();
}
