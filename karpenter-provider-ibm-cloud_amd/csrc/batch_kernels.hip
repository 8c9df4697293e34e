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

// the first-pass queue records of n problems (after their uploads): two launches
extern "C" hipError_t gsk_queue_records_batch(const DevProblem* ds, uint32_t n, uint32_t max_pods, hipStream_t s) {
  if (!n || !max_pods) return hipSuccess;
  if (n > 65535) return hipErrorInvalidValue;
  const uint32_t blocks = (max_pods + 255) / 256;
  hipLaunchKernelGGL(queue_records_kernel_batch, dim3(blocks, n), dim3(256), 0, s, ds);
  hipLaunchKernelGGL(queue_runs_kernel_batch, dim3(blocks, n), dim3(256), 0, s, ds);
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
// The instantiations live in ffd_wave_batch_r.hip, one translation unit per
// (R, TOPO): each exports its launcher and its LDS attribute setter.
#define GSK_DECL(n, t)                                                                                      \
  extern "C" hipError_t gsk_ffdwb_launch_r##n##_t##t(const DevProblem* ds, uint32_t cnt, uint32_t wide, uint32_t lds, \
                                                     hipStream_t s);                                        \
  extern "C" hipError_t gsk_ffdwb_attr_r##n##_t##t(uint32_t lds_total, uint32_t* dyn_min);
#define GSK_DECL2(n) GSK_DECL(n, 0) GSK_DECL(n, 1)
GSK_DECL2(1) GSK_DECL2(2) GSK_DECL2(3) GSK_DECL2(4) GSK_DECL2(5) GSK_DECL2(6) GSK_DECL2(7) GSK_DECL2(8)
#undef GSK_DECL2
#undef GSK_DECL
static uint32_t g_ffdwb_dyn_max = 0;

extern "C" hipError_t gsk_init_ffdw_batch(uint32_t lds_total) {
  hipError_t e = hipSuccess;
  uint32_t dmin = 0;
#define GSK_ATTR(n, t) \
  if (hipError_t x = gsk_ffdwb_attr_r##n##_t##t(lds_total, &dmin); x != hipSuccess) e = x;
#define GSK_ATTR2(n) GSK_ATTR(n, 0) GSK_ATTR(n, 1)
  GSK_ATTR2(1) GSK_ATTR2(2) GSK_ATTR2(3) GSK_ATTR2(4) GSK_ATTR2(5) GSK_ATTR2(6) GSK_ATTR2(7) GSK_ATTR2(8)
#undef GSK_ATTR2
#undef GSK_ATTR
  g_ffdwb_dyn_max = dmin;
  return e;
}

extern "C" uint32_t gsk_ffdw_batch_dyn_lds_max(void) { return g_ffdwb_dyn_max; }

// n problems of one instantiation (R resources, the general variant or not,
// wide option rows or not), one workgroup each: one launch.  lds: the largest
// dynamic LDS among them (gsk_ffdw's formula per problem).
extern "C" hipError_t gsk_ffdw_batch(const DevProblem* ds, uint32_t n, uint32_t R, uint32_t topo, uint32_t wide,
                                     uint32_t lds, hipStream_t s) {
  if (!n || lds > g_ffdwb_dyn_max) return hipErrorInvalidConfiguration;
  switch (R * 2 + (topo ? 1 : 0)) {
#define GSK_CASE(k)                                                    \
  case 2 * k: return gsk_ffdwb_launch_r##k##_t0(ds, n, wide, lds, s); \
  case 2 * k + 1: return gsk_ffdwb_launch_r##k##_t1(ds, n, wide, lds, s);
    GSK_CASE(1) GSK_CASE(2) GSK_CASE(3) GSK_CASE(4) GSK_CASE(5) GSK_CASE(6) GSK_CASE(7) GSK_CASE(8)
#undef GSK_CASE
    default:
      return hipErrorInvalidValue;
  }
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

// The instantiations of the batched simulation kernel live in
// ffd_sim_batch_r.hip, one translation unit per (R, TOPO): each exports its
// launcher, its LDS attribute setter and its occupancy query.
#define GSK_DECL(n, t)                                                                                                  \
  extern "C" hipError_t gsk_ffdsb_launch_r##n##_t##t(const DevProblem* ds, const uint32_t* blocks, uint32_t cnt,        \
                                                     uint32_t max_blocks, uint32_t nt, uint32_t lds, uint32_t ov_epoch, \
                                                     hipStream_t s);                                                    \
  extern "C" hipError_t gsk_ffdsb_attr_r##n##_t##t(uint32_t lds_total, uint32_t* dyn_min);                              \
  extern "C" uint32_t gsk_ffdsb_occ_r##n##_t##t(uint32_t nt, uint32_t lds);
#define GSK_DECL2(n) GSK_DECL(n, 0) GSK_DECL(n, 1)
GSK_DECL2(1) GSK_DECL2(2) GSK_DECL2(3) GSK_DECL2(4) GSK_DECL2(5) GSK_DECL2(6) GSK_DECL2(7) GSK_DECL2(8)
#undef GSK_DECL2
#undef GSK_DECL
static uint32_t g_ffdsb_dyn_max = 0;

extern "C" hipError_t gsk_init_ffd_sim_batch(uint32_t lds_total) {
  hipError_t e = hipSuccess;
  uint32_t dmin = 0;
#define GSK_ATTR(n, t) \
  if (hipError_t x = gsk_ffdsb_attr_r##n##_t##t(lds_total, &dmin); x != hipSuccess) e = x;
#define GSK_ATTR2(n) GSK_ATTR(n, 0) GSK_ATTR(n, 1)
  GSK_ATTR2(1) GSK_ATTR2(2) GSK_ATTR2(3) GSK_ATTR2(4) GSK_ATTR2(5) GSK_ATTR2(6) GSK_ATTR2(7) GSK_ATTR2(8)
#undef GSK_ATTR2
#undef GSK_ATTR
  g_ffdsb_dyn_max = dmin;
  return e;
}

extern "C" uint32_t gsk_ffd_sim_batch_dyn_lds_max(void) { return g_ffdsb_dyn_max; }

// resident workgroups per CU of the batched simulation kernel (R resources,
// the general variant or not, nt threads) at a dynamic LDS size; at least 1
extern "C" uint32_t gsk_ffd_sim_batch_blocks_per_cu(uint32_t R, uint32_t lds, uint32_t nt, uint32_t general) {
  uint32_t n = 0;
  switch (R * 2 + (general ? 1 : 0)) {
#define GSK_CASE(k)                                      \
  case 2 * k: n = gsk_ffdsb_occ_r##k##_t0(nt, lds); break; \
  case 2 * k + 1: n = gsk_ffdsb_occ_r##k##_t1(nt, lds); break;
    GSK_CASE(1) GSK_CASE(2) GSK_CASE(3) GSK_CASE(4) GSK_CASE(5) GSK_CASE(6) GSK_CASE(7) GSK_CASE(8)
#undef GSK_CASE
  }
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
  switch (R * 2 + (general ? 1 : 0)) {
#define GSK_CASE(k)                                                                                \
  case 2 * k: return gsk_ffdsb_launch_r##k##_t0(ds, blocks, n, max_blocks, nt, lds, ov_epoch, s); \
  case 2 * k + 1: return gsk_ffdsb_launch_r##k##_t1(ds, blocks, n, max_blocks, nt, lds, ov_epoch, s);
    GSK_CASE(1) GSK_CASE(2) GSK_CASE(3) GSK_CASE(4) GSK_CASE(5) GSK_CASE(6) GSK_CASE(7) GSK_CASE(8)
#undef GSK_CASE
    default:
      return hipErrorInvalidValue;
  }
}
