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

// dynamic LDS: slack + room u64, ord/sc/scr u16, tmpl u8 per claim, thresholds,
// (simulations) the touched-node bitmap, and the topology
// spread state (known domains, per-pod minimum, zone counts) of TG groups
extern "C" uint32_t gsk_ffd_lds_bytes(uint32_t max_claims, uint32_t nthr, uint32_t nb_words,
                                      uint32_t topo_bytes) {
  const uint32_t thr = nthr + 4;
  const uint32_t base = (((23u * max_claims + 7u) & ~7u) + thr * 8u + nb_words * 4u + 7u) & ~7u;
  return base + topo_bytes;
}

// every instantiation may use all LDS its static footprint leaves free
static uint32_t g_ffd_dyn_max = 0;

template <uint32_t RR, bool SIM, bool TOPO = false, uint32_t NT = SIM ? FB_SIM : FB_MAX>
static hipError_t ffd_attr(uint32_t lds_total) {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, (const void*)ffd_kernel<RR, SIM, NT, TOPO>);
  if (e != hipSuccess) return e;
  const uint32_t dyn = lds_total > a.sharedSizeBytes ? lds_total - (uint32_t)a.sharedSizeBytes : 0;
  if (!g_ffd_dyn_max || dyn < g_ffd_dyn_max) g_ffd_dyn_max = dyn;
  return hipFuncSetAttribute((const void*)ffd_kernel<RR, SIM, NT, TOPO>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)dyn);
}

template <uint32_t RR>
static hipError_t ffd_attr_all(uint32_t lds_total) {
  hipError_t e = hipSuccess;
  for (hipError_t x : {ffd_attr<RR, false>(lds_total), ffd_attr<RR, false, true>(lds_total), ffd_attr<RR, true>(lds_total),
                       ffd_attr<RR, true, false, FB_SIM_NARROW>(lds_total), ffd_attr<RR, true, true, FB_SIM>(lds_total),
                       ffd_attr<RR, true, true, FB_SIM_NARROW>(lds_total)})
    if (x != hipSuccess) e = x;
  return e;
}

extern "C" hipError_t gsk_init_ffd(uint32_t lds_total) {
  hipError_t e = hipSuccess;
  for (hipError_t x : {ffd_attr_all<1>(lds_total), ffd_attr_all<2>(lds_total), ffd_attr_all<3>(lds_total),
                       ffd_attr_all<4>(lds_total), ffd_attr_all<5>(lds_total), ffd_attr_all<6>(lds_total),
                       ffd_attr_all<7>(lds_total), ffd_attr_all<8>(lds_total)})
    if (x != hipSuccess) e = x;
  return e;
}

extern "C" uint32_t gsk_ffd_dyn_lds_max(void) { return g_ffd_dyn_max; }

// resident simulation workgroups per CU for a given dynamic LDS size
template <uint32_t RR>
static hipError_t sim_occ(int* n, bool narrow, bool general, uint32_t lds) {
  if (general)
    return narrow ? hipOccupancyMaxActiveBlocksPerMultiprocessor(n, (const void*)ffd_kernel<RR, true, FB_SIM_NARROW, true>,
                                                                 FB_SIM_NARROW, lds)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(n, (const void*)ffd_kernel<RR, true, FB_SIM, true>, FB_SIM, lds);
  return narrow ? hipOccupancyMaxActiveBlocksPerMultiprocessor(n, (const void*)ffd_kernel<RR, true, FB_SIM_NARROW, false>,
                                                               FB_SIM_NARROW, lds)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(n, (const void*)ffd_kernel<RR, true, FB_SIM, false>, FB_SIM, lds);
}

extern "C" uint32_t gsk_ffd_sim_blocks_per_cu(uint32_t R, uint32_t lds, uint32_t nt, uint32_t general) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  const bool narrow = nt == (uint32_t)FB_SIM_NARROW;
  switch (R) {
#define GSK_OCC(k) \
  case k: e = sim_occ<k>(&n, narrow, general != 0, lds); break;
    GSK_OCC(1) GSK_OCC(2) GSK_OCC(3) GSK_OCC(4) GSK_OCC(5) GSK_OCC(6) GSK_OCC(7) GSK_OCC(8)
#undef GSK_OCC
  }
  return e == hipSuccess && n > 0 ? (uint32_t)n : 1u;
}

// grid: 1 workgroup (provisioning Solve) or `blocks` persistent workgroups
// draining the simulation counter (consolidation)
extern "C" hipError_t gsk_ffd(const DevProblem* d, uint32_t blocks, hipStream_t s) {
  const uint32_t lds = gsk_ffd_lds_bytes(d->max_claims, d->n_thr, d->nb_words, topo_lds_bytes(d->TGZ, d->ZS, d->TGH, d->n_lazy)) +
                       (d->n_sims ? 8u * d->ovh_slots + (d->sim_lds ? 32u * d->max_claims : 0u) : 0u);
  if (lds > g_ffd_dyn_max) return hipErrorInvalidConfiguration;
  const bool sim = d->n_sims > 0;
  // shape: 0 provisioning, 1 provisioning (general variant), 2 simulations, 3 narrow simulations,
  // 4 / 5 simulations / narrow simulations, general variant (topology groups, volumes, minValues)
  if (sim && d->sim_nt != (uint32_t)FB_SIM && d->sim_nt != (uint32_t)FB_SIM_NARROW) return hipErrorInvalidValue;
  const bool general = d->TG || d->any_mv || d->any_vol;
  const uint32_t shape = sim ? (d->sim_nt == (uint32_t)FB_SIM_NARROW ? 3u : 2u) + (general ? 2u : 0u) : (general ? 1u : 0u);
  switch (d->R * 8 + shape) {
#define GSK_CASE(n)                                                                                          \
  case 8 * n: hipLaunchKernelGGL((ffd_kernel<n, false, FB_MAX, false>), dim3(1), dim3(FB_MAX), lds, s, *d); break; \
  case 8 * n + 1: hipLaunchKernelGGL((ffd_kernel<n, false, FB_MAX, true>), dim3(1), dim3(FB_MAX), lds, s, *d); break; \
  case 8 * n + 2: hipLaunchKernelGGL((ffd_kernel<n, true, FB_SIM, false>), dim3(blocks), dim3(FB_SIM), lds, s, *d); break; \
  case 8 * n + 3:                                                                                            \
    hipLaunchKernelGGL((ffd_kernel<n, true, FB_SIM_NARROW, false>), dim3(blocks), dim3(FB_SIM_NARROW), lds, s, *d); \
    break;                                                                                                    \
  case 8 * n + 4: hipLaunchKernelGGL((ffd_kernel<n, true, FB_SIM, true>), dim3(blocks), dim3(FB_SIM), lds, s, *d); break; \
  case 8 * n + 5:                                                                                            \
    hipLaunchKernelGGL((ffd_kernel<n, true, FB_SIM_NARROW, true>), dim3(blocks), dim3(FB_SIM_NARROW), lds, s, *d); \
    break;
    GSK_CASE(1) GSK_CASE(2) GSK_CASE(3) GSK_CASE(4) GSK_CASE(5) GSK_CASE(6) GSK_CASE(7) GSK_CASE(8)
#undef GSK_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// the first-pass queue record kernels (shared with the batched kernels of batch_kernels.hip)
#include "queue_kernels.hpp"

extern "C" hipError_t gsk_queue_records(const DevProblem* d, hipStream_t s) {
  if (!d->P) return hipSuccess;
  hipLaunchKernelGGL(queue_records_kernel, dim3((d->P + 255) / 256), dim3(256), 0, s, *d);
  return hipGetLastError();
}
