// ffd_wave_r.hip — the instantiations of ffdw_kernel (ffd_wave.hpp) for one
// resource count GS_WAVE_R and one variant GS_WAVE_TOPO (0: the plain
// variant, 1: the general one), with the claim scan state in LDS (register
// mode) or in HBM (ch), for narrow and wide option rows: compiled once per (R, TOPO) so the large register-
// mode bodies build in parallel (Makefile ffd_wave_r<R>_t<T>.o).
#include "ffd_wave.hpp"
#include "kernel_api.hpp"

#ifndef GS_WAVE_R
#error "GS_WAVE_R (1..8) and GS_WAVE_TOPO (0/1) select the instantiation"
#endif

using namespace gsd;

template <bool CH, bool WIDE>
static const void* ffdw_fn() {
  return (const void*)ffdw_kernel<GS_WAVE_R, GS_WAVE_TOPO != 0, CH, WIDE>;
}

static hipError_t ffdw_set_lds(uint32_t lds_total, uint32_t* dyn_min) {
  const hipError_t e[4] = {
      set_max_dyn_lds(ffdw_fn<false, false>(), lds_total, dyn_min), set_max_dyn_lds(ffdw_fn<true, false>(), lds_total, dyn_min),
      set_max_dyn_lds(ffdw_fn<false, true>(), lds_total, dyn_min), set_max_dyn_lds(ffdw_fn<true, true>(), lds_total, dyn_min)};
  for (hipError_t x : e)
    if (x != hipSuccess) return x;
  return hipSuccess;
}

// mode: bit 0 = claim scan state in HBM, bit 1 = wide option rows (layout.hpp wide_rows)
static hipError_t ffdw_launch(const DevProblem* d, uint32_t mode, uint32_t lds, hipStream_t s) {
  constexpr bool T = GS_WAVE_TOPO != 0;
  switch (mode & 3u) {
    case 0: hipLaunchKernelGGL((ffdw_kernel<GS_WAVE_R, T, false, false>), dim3(1), dim3(128), lds, s, *d); break;
    case 1: hipLaunchKernelGGL((ffdw_kernel<GS_WAVE_R, T, true, false>), dim3(1), dim3(128), lds, s, *d); break;
    case 2: hipLaunchKernelGGL((ffdw_kernel<GS_WAVE_R, T, false, true>), dim3(1), dim3(128), lds, s, *d); break;
    default: hipLaunchKernelGGL((ffdw_kernel<GS_WAVE_R, T, true, true>), dim3(1), dim3(128), lds, s, *d); break;
  }
  return hipGetLastError();
}

extern "C" const GskWaveFamily* GSK_RT_NAME(gsk_ffdw, GS_WAVE_R, GS_WAVE_TOPO)(void) {
  static const GskWaveFamily f = {GS_WAVE_R, GS_WAVE_TOPO, ffdw_launch, ffdw_set_lds};
  return &f;
}
