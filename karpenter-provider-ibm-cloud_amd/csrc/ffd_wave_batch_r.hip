// ffd_wave_batch_r.hip — the batched instantiations of the single-wave Solve
// (ffd_wave.hpp, GS_WAVE_BATCH): one workgroup per problem of a device array
// of DevProblem, for one resource count GS_WAVE_R and one variant
// GS_WAVE_TOPO, claim scan state in LDS only (a problem that outgrows it
// reruns alone through gs_run), narrow and wide option rows.  Compiled once
// per (R, TOPO) next to ffd_wave_r.hip (Makefile ffd_wave_batch_r<R>_t<T>.o).
#define GS_WAVE_BATCH 1
#include "ffd_wave.hpp"
#include "kernel_api.hpp"

#ifndef GS_WAVE_R
#error "GS_WAVE_R (1..8) and GS_WAVE_TOPO (0/1) select the instantiation"
#endif

using namespace gsd;

template <bool WIDE>
static const void* ffdwb_fn() {
  return (const void*)ffdw_batch_kernel<GS_WAVE_R, GS_WAVE_TOPO != 0, false, WIDE>;
}

static hipError_t ffdwb_set_lds(uint32_t lds_total, uint32_t* dyn_min) {
  const hipError_t e[2] = {set_max_dyn_lds(ffdwb_fn<false>(), lds_total, dyn_min),
                           set_max_dyn_lds(ffdwb_fn<true>(), lds_total, dyn_min)};
  for (hipError_t x : e)
    if (x != hipSuccess) return x;
  return hipSuccess;
}

// n problems at ds, one workgroup each; lds: the largest problem's dynamic LDS
// (every workgroup lays its own out from its problem's sizes)
static hipError_t ffdwb_launch(const DevProblem* ds, uint32_t n, uint32_t wide, uint32_t lds, hipStream_t s) {
  constexpr bool T = GS_WAVE_TOPO != 0;
  if (wide)
    hipLaunchKernelGGL((ffdw_batch_kernel<GS_WAVE_R, T, false, true>), dim3(n), dim3(128), lds, s, ds);
  else
    hipLaunchKernelGGL((ffdw_batch_kernel<GS_WAVE_R, T, false, false>), dim3(n), dim3(128), lds, s, ds);
  return hipGetLastError();
}

extern "C" const GskWaveBatchFamily* GSK_RT_NAME(gsk_ffdwb, GS_WAVE_R, GS_WAVE_TOPO)(void) {
  static const GskWaveBatchFamily f = {GS_WAVE_R, GS_WAVE_TOPO, ffdwb_launch, ffdwb_set_lds};
  return &f;
}
