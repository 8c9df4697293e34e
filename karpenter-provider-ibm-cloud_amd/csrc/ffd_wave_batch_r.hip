// ffd_wave_batch_r.hip — the batched instantiations of the single-wave Solve
// (ffd_wave.hpp, GS_WAVE_BATCH): one workgroup per problem of a device array
// of DevProblem, for one resource count GS_WAVE_R and one variant
// GS_WAVE_TOPO, claim scan state in LDS only (a problem that outgrows it
// reruns alone through gs_run), narrow and wide option rows.  Compiled once
// per (R, TOPO) next to ffd_wave_r.hip (Makefile ffd_wave_batch_r<R>_t<T>.o).
#define GS_WAVE_BATCH 1
#include "ffd_wave.hpp"

#ifndef GS_WAVE_R
#error "GS_WAVE_R (1..8) and GS_WAVE_TOPO (0/1) select the instantiation"
#endif

using namespace gsd;

#define GSK_CAT2(a, b, c, d) a##b##c##d
#define GSK_CAT(a, b, c, d) GSK_CAT2(a, b, c, d)
#define GSK_LAUNCH GSK_CAT(gsk_ffdwb_launch_r, GS_WAVE_R, _t, GS_WAVE_TOPO)
#define GSK_ATTR GSK_CAT(gsk_ffdwb_attr_r, GS_WAVE_R, _t, GS_WAVE_TOPO)

template <bool WIDE>
static hipError_t ffdwb_attr_one(uint32_t lds_total, uint32_t* dyn_min) {
  const void* fn = (const void*)ffdw_batch_kernel<GS_WAVE_R, GS_WAVE_TOPO != 0, false, WIDE>;
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, fn);
  if (e != hipSuccess) return e;
  const uint32_t dyn = lds_total > a.sharedSizeBytes ? lds_total - (uint32_t)a.sharedSizeBytes : 0;
  if (!*dyn_min || dyn < *dyn_min) *dyn_min = dyn;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
}

extern "C" hipError_t GSK_ATTR(uint32_t lds_total, uint32_t* dyn_min) {
  const hipError_t e[2] = {ffdwb_attr_one<false>(lds_total, dyn_min), ffdwb_attr_one<true>(lds_total, dyn_min)};
  for (hipError_t x : e)
    if (x != hipSuccess) return x;
  return hipSuccess;
}

// n problems at ds, one workgroup each; lds: the largest problem's dynamic LDS
// (every workgroup lays its own out from its problem's sizes)
extern "C" hipError_t GSK_LAUNCH(const DevProblem* ds, uint32_t n, uint32_t wide, uint32_t lds, hipStream_t s) {
  constexpr bool T = GS_WAVE_TOPO != 0;
  if (wide)
    hipLaunchKernelGGL((ffdw_batch_kernel<GS_WAVE_R, T, false, true>), dim3(n), dim3(128), lds, s, ds);
  else
    hipLaunchKernelGGL((ffdw_batch_kernel<GS_WAVE_R, T, false, false>), dim3(n), dim3(128), lds, s, ds);
  return hipGetLastError();
}
