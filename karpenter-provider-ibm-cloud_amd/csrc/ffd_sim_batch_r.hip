// ffd_sim_batch_r.hip — the batched instantiations of the simulation kernel
// (ffd_block.hpp, GS_SIM_BATCH): the persistent simulation workgroups of many
// consolidation problems in one launch, for one resource count GS_SIM_R and
// one variant GS_SIM_TOPO, in the wide (FB_SIM) and the narrow
// (FB_SIM_NARROW) shape.  Compiled once per (R, TOPO)
// (Makefile ffd_sim_batch_r<R>_t<T>.o); batch_kernels.hip dispatches.
#define GS_SIM_BATCH 1
#include "ffd_block.hpp"

#ifndef GS_SIM_R
#error "GS_SIM_R (1..8) and GS_SIM_TOPO (0/1) select the instantiation"
#endif

#define GSK_CAT2(a, b, c, d) a##b##c##d
#define GSK_CAT(a, b, c, d) GSK_CAT2(a, b, c, d)
#define GSK_LAUNCH GSK_CAT(gsk_ffdsb_launch_r, GS_SIM_R, _t, GS_SIM_TOPO)
#define GSK_ATTR GSK_CAT(gsk_ffdsb_attr_r, GS_SIM_R, _t, GS_SIM_TOPO)
#define GSK_OCC GSK_CAT(gsk_ffdsb_occ_r, GS_SIM_R, _t, GS_SIM_TOPO)

template <uint32_t NT>
static const void* ffdsb_fn() {
  return (const void*)ffd_sim_batch_kernel<GS_SIM_R, true, NT, GS_SIM_TOPO != 0>;
}

template <uint32_t NT>
static hipError_t ffdsb_attr_one(uint32_t lds_total, uint32_t* dyn_min) {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, ffdsb_fn<NT>());
  if (e != hipSuccess) return e;
  const uint32_t dyn = lds_total > a.sharedSizeBytes ? lds_total - (uint32_t)a.sharedSizeBytes : 0;
  if (!*dyn_min || dyn < *dyn_min) *dyn_min = dyn;
  return hipFuncSetAttribute(ffdsb_fn<NT>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
}

// every instantiation may use all LDS its static footprint leaves free
extern "C" hipError_t GSK_ATTR(uint32_t lds_total, uint32_t* dyn_min) {
  const hipError_t e[2] = {ffdsb_attr_one<FB_SIM>(lds_total, dyn_min), ffdsb_attr_one<FB_SIM_NARROW>(lds_total, dyn_min)};
  for (hipError_t x : e)
    if (x != hipSuccess) return x;
  return hipSuccess;
}

// resident workgroups per CU at a dynamic LDS size (0: the query failed)
extern "C" uint32_t GSK_OCC(uint32_t nt, uint32_t lds) {
  int n = 0;
  const hipError_t e = nt == (uint32_t)FB_SIM_NARROW
                           ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ffdsb_fn<FB_SIM_NARROW>(), FB_SIM_NARROW, lds)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ffdsb_fn<FB_SIM>(), FB_SIM, lds);
  return e == hipSuccess && n > 0 ? (uint32_t)n : 0u;
}

// n problems at ds with blocks[i] workgroups each (max_blocks the largest);
// lds: the largest problem's dynamic LDS (every workgroup lays its own out
// from its problem's sizes)
extern "C" hipError_t GSK_LAUNCH(const DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t max_blocks, uint32_t nt,
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
