// ffd_sim_batch_r.hip — the batched instantiations of the simulation kernel
// (ffd_block.hpp, GS_SIM_BATCH): the persistent simulation workgroups of many
// consolidation problems in one launch, for one resource count GS_SIM_R and
// one variant GS_SIM_TOPO, in the wide (FB_SIM) and the narrow
// (FB_SIM_NARROW) shape.  Compiled once per (R, TOPO)
// (Makefile ffd_sim_batch_r<R>_t<T>.o); batch_kernels.hip dispatches.
#define GS_SIM_BATCH 1
#include "ffd_block.hpp"
#include "kernel_api.hpp"

#ifndef GS_SIM_R
#error "GS_SIM_R (1..8) and GS_SIM_TOPO (0/1) select the instantiation"
#endif

template <uint32_t NT>
static const void* ffdsb_fn() {
  return (const void*)ffd_sim_batch_kernel<GS_SIM_R, true, NT, GS_SIM_TOPO != 0>;
}

static hipError_t ffdsb_set_lds(uint32_t lds_total, uint32_t* dyn_min) {
  const hipError_t e[2] = {set_max_dyn_lds(ffdsb_fn<FB_SIM>(), lds_total, dyn_min),
                           set_max_dyn_lds(ffdsb_fn<FB_SIM_NARROW>(), lds_total, dyn_min)};
  for (hipError_t x : e)
    if (x != hipSuccess) return x;
  return hipSuccess;
}

// resident workgroups per CU at a dynamic LDS size (0: the query failed)
static uint32_t ffdsb_blocks_per_cu(uint32_t nt, uint32_t lds) {
  int n = 0;
  const hipError_t e = nt == (uint32_t)FB_SIM_NARROW
                           ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ffdsb_fn<FB_SIM_NARROW>(), FB_SIM_NARROW, lds)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ffdsb_fn<FB_SIM>(), FB_SIM, lds);
  return e == hipSuccess && n > 0 ? (uint32_t)n : 0u;
}

// n problems at ds with blocks[i] workgroups each (max_blocks the largest);
// lds: the largest problem's dynamic LDS (every workgroup lays its own out
// from its problem's sizes)
static hipError_t ffdsb_launch(const DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t max_blocks, uint32_t nt,
                                uint32_t lds, uint32_t ov_epoch, hipStream_t s) {
  constexpr bool T = GS_SIM_TOPO != 0;
  if (nt == (uint32_t)FB_SIM_NARROW)
    hipLaunchKernelGGL((ffd_sim_batch_kernel<GS_SIM_R, true, FB_SIM_NARROW, T>), dim3(max_blocks, n), dim3(FB_SIM_NARROW), lds,
                       s, ds, blocks, ov_epoch);
  else
    hipLaunchKernelGGL((ffd_sim_batch_kernel<GS_SIM_R, true, FB_SIM, T>), dim3(max_blocks, n), dim3(FB_SIM), lds, s, ds,
                       blocks, ov_epoch);
  return hipGetLastError();
}

extern "C" const GskSimBatchFamily* GSK_RT_NAME(gsk_ffdsb, GS_SIM_R, GS_SIM_TOPO)(void) {
  static const GskSimBatchFamily f = {GS_SIM_R, GS_SIM_TOPO, ffdsb_launch, ffdsb_set_lds, ffdsb_blocks_per_cu};
  return &f;
}
