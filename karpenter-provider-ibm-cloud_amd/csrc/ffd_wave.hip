// ffd_wave.hip — K4 provisioning Solve as ONE wave: the state reset kernel,
// the launcher (the kernel template is in ffd_wave.hpp, its instantiations
// in ffd_wave_r.hip) and the autoplacement ranking sort.
#include "ffd_wave.hpp"
#include "kernel_api.hpp"

using namespace gsd;

// the Solve's state reset (shared with the batched kernels of batch_kernels.hip)
#include "init_kernel.hpp"


// ---------------------------------------------------------------- launchers
// The kernel instantiations live in ffd_wave_r.hip, one translation unit per
// (R, TOPO): each exports its family record (kernel_api.hpp).
static auto& ffdw_families() {
#define GSK_ENTRY(r, t) GSK_RT_NAME(gsk_ffdw, r, t)(),
  static const GskWaveFamily* const table[] = {GSK_FOR_EACH_RT(GSK_ENTRY)};
#undef GSK_ENTRY
  return table;
}
static uint32_t g_ffdw_dyn_max = 0;

extern "C" hipError_t gsk_init_ffdw(uint32_t lds_total) { return gsk_set_lds(ffdw_families(), lds_total, &g_ffdw_dyn_max); }

extern "C" uint32_t gsk_ffdw_dyn_lds_max(void) { return g_ffdw_dyn_max; }

// the single-wave provisioning Solve: grid-wide state reset, then one wave;
// ch: the claim scan state in HBM (d->ch_* allocated, claim_cap slots)
extern "C" hipError_t gsk_ffdw(const DevProblem* d, uint32_t ch, hipStream_t s) {
  const uint32_t lds = wave_lds_bytes(*d, ch != 0);
  if (lds > g_ffdw_dyn_max) return hipErrorInvalidConfiguration;
  if (d->n_sims) return hipErrorInvalidValue;
  if (ch && !(d->ch_slk && d->ch_rm && d->ch_so && d->ch_scr && d->ch_tmpl)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ffd_init_kernel, dim3(256), dim3(256), 0, s, *d);
  const GskWaveFamily* f = gsk_family(ffdw_families(), d->R, general_variant(*d));
  if (!f) return hipErrorInvalidValue;
  return f->launch(d, (ch ? 1u : 0u) | (wide_rows(d->W) ? 2u : 0u), lds, s);
}

// ------------------------------------------------ autoplacement ranking sort
// gs_rank_instance_types (rank.hip) sorts its kept instance types with the
// single-wave sort.Slice restatement above (WaveSort: every partition step a
// ballot, no workgroup barrier).  keys[k] = how many kept scores are strictly
// below score k: the same Less outcomes as the float64 compare (NaN refused
// on the host), so the permutation is the reference's.  pos[k] = compacted
// position; both sorted in place.  *np = the kept count (written by
// rank_kernel on the same stream); cap bounds it (<= GS_RANK_MAX).
extern "C" __global__ __launch_bounds__(64) void rank_sort_kernel(uint16_t* keys, uint16_t* pos, const uint32_t* np,
                                                                  uint32_t cap, int x) {
  extern __shared__ uint32_t rs_lds[];  // so[cap] (key | position << 16) | scr u16[cap + 2]
  __shared__ Frame rs_stk[64];
  const uint32_t n = __builtin_amdgcn_readfirstlane(*np <= cap ? *np : 0u);
  const uint32_t lane = threadIdx.x;
  lds_u32* so = (lds_u32*)rs_lds;
  lds_u16* scr = (lds_u16*)(rs_lds + cap);
  for (uint32_t k = lane; k < n; k += 64) so[k] = (uint32_t)keys[k] | ((uint32_t)pos[k] << 16);
  wsync();
  wave_pdqsort<GS_WAVE_SEQ, lds_u32, lds_u16, false, true>(so, scr, (lds_frame*)rs_stk, lane, (n + 1) / 2, (int)n,
                                                          x < (int)n ? x : -1);
  for (uint32_t k = lane; k < n; k += 64) {
    const uint32_t x = so[k];
    keys[k] = (uint16_t)(x & 0xFFFFu);
    pos[k] = (uint16_t)(x >> 16);
  }
}

// x: a position known to be the only one out of order (the test hook's
// one-change inputs take WaveSort::partition_known, as the Solve's do), or
// -1 (the ranking)
extern "C" hipError_t gsk_rank_sort(uint16_t* keys, uint16_t* pos, const uint32_t* np, uint32_t cap, int x, hipStream_t s) {
  const size_t lds = (size_t)cap * sizeof(uint32_t) + (size_t)(cap + 2) * sizeof(uint16_t);
  hipLaunchKernelGGL(rank_sort_kernel, dim3(1), dim3(64), lds, s, keys, pos, np, cap, x);
  return hipGetLastError();
}

