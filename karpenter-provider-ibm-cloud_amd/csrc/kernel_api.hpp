// kernel_api.hpp — the launch interface between the host side and the units
// that hold kernels: every gsk_* launcher, declared once.  The host includes it
// through ctx.hpp; every unit that defines a gsk_* symbol includes it too, so a
// definition that differs from its declaration does not compile (C linkage
// makes it a conflicting declaration).  The rules the launchers and the host
// share (variant, wide rows, dynamic LDS) are in layout.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_family.hpp"
#include "layout.hpp"

extern "C" {
// kernels.hip: K1/K2, K3, the minValues rows and the shard merge
hipError_t gsk_init_trunc(uint32_t trunc_lds_bytes);
hipError_t gsk_feas(const gsd::DevProblem* d, uint32_t static_mode, uint32_t w_lo, uint32_t w_hi, hipStream_t s);
hipError_t gsk_trunc(const gsd::DevProblem* d, uint32_t lds_bytes, uint32_t n_slots, hipStream_t s);
hipError_t gsk_trunc_slots(const gsd::DevProblem* d, uint32_t lds_bytes, uint32_t slot0, uint32_t n_slots, hipStream_t s);
hipError_t gsk_mv_rows(const gsd::DevProblem* d, hipStream_t s);
hipError_t gsk_merge_shards(const gsd::ShardMerge* m, hipStream_t s);
// ffd.hip: the block Solve and the consolidation simulations
hipError_t gsk_init_ffd(uint32_t lds_total);
uint32_t gsk_ffd_dyn_lds_max(void);
uint32_t gsk_ffd_sim_blocks_per_cu(uint32_t R, uint32_t lds, uint32_t nt, uint32_t general);
hipError_t gsk_ffd(const gsd::DevProblem* d, uint32_t blocks, hipStream_t s);
hipError_t gsk_queue_records(const gsd::DevProblem* d, hipStream_t s);
// ffd_wave.hip: the single-wave Solve and the ranking sort
hipError_t gsk_init_ffdw(uint32_t lds_total);
uint32_t gsk_ffdw_dyn_lds_max(void);
hipError_t gsk_ffdw(const gsd::DevProblem* d, uint32_t ch, hipStream_t s);
hipError_t gsk_rank_sort(uint16_t* keys, uint16_t* pos, const uint32_t* np, uint32_t cap, int x, hipStream_t s);
// batch_kernels.hip: the grid kernels over a device array of problems
hipError_t gsk_init_batch(uint32_t trunc_lds_bytes);
uint32_t gsk_feas_lp(uint32_t W);
hipError_t gsk_feas_batch(const gsd::DevProblem* ds, uint32_t n, uint32_t lp, uint64_t max_cursors, uint64_t max_pairs,
                          hipStream_t s);
hipError_t gsk_init_state_batch(const gsd::DevProblem* ds, uint32_t n, hipStream_t s);
hipError_t gsk_queue_records_batch(const gsd::DevProblem* ds, uint32_t n, uint32_t max_pods, hipStream_t s);
hipError_t gsk_init_ffdw_batch(uint32_t lds_total);
uint32_t gsk_ffdw_batch_dyn_lds_max(void);
hipError_t gsk_ffdw_batch(const gsd::DevProblem* ds, uint32_t n, uint32_t R, uint32_t topo, uint32_t wide, uint32_t lds,
                          hipStream_t s);
hipError_t gsk_trunc_batch(const gsd::DevProblem* ds, uint32_t n, uint32_t max_slots, uint32_t lds_bytes, hipStream_t s);
// ... and the consolidation simulations of a device array of problems
hipError_t gsk_init_ffd_sim_batch(uint32_t lds_total);
uint32_t gsk_ffd_sim_batch_dyn_lds_max(void);
uint32_t gsk_ffd_sim_batch_blocks_per_cu(uint32_t R, uint32_t lds, uint32_t nt, uint32_t general);
hipError_t gsk_sim_begin_batch(const gsd::DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t clear_overlays,
                               hipStream_t s);
hipError_t gsk_ffd_sim_batch(const gsd::DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t max_blocks, uint32_t R,
                             uint32_t general, uint32_t nt, uint32_t lds, uint32_t ov_epoch, hipStream_t s);
hipError_t gsk_trunc_sims_batch(const gsd::DevProblem* ds, uint32_t n, uint32_t mv, uint32_t max_sims, uint32_t max_slots,
                                uint32_t lds_bytes, hipStream_t s);
hipError_t gsk_cons_gather_batch(const gsd::DevProblem* ds, const uint32_t* blocks, const uint32_t* sim_base, uint32_t n,
                                 uint32_t max_sims, gsd::SlotOut* slots, gsd::SimOut* recs, gsd::OptPair* opts,
                                 uint32_t* cursor, hipStream_t s);
// batch_fetch.hip: the records of n problems of a device array, packed into `staging`
hipError_t gsk_fetch_gather_batch(const gsd::DevProblem* ds, uint32_t n, uint32_t max_pods, void* staging,
                                  uint64_t payload_cap, hipStream_t s);
}  // extern "C"

// The per-(R, TOPO) units export one function per family, which returns the
// family's record (kernel_family.hpp).
// set_lds: gives every instantiation of the family the LDS its static
// footprint leaves free of lds_total (set_max_dyn_lds).
// ffd_wave_r.hip; mode: bit 0 = claim scan state in HBM, bit 1 = wide option rows
struct GskWaveFamily {
  uint32_t R, general;
  hipError_t (*launch)(const gsd::DevProblem* d, uint32_t mode, uint32_t lds, hipStream_t s);
  hipError_t (*set_lds)(uint32_t lds_total, uint32_t* dyn_min);
};
// ffd_wave_batch_r.hip: n problems at ds, one workgroup each
struct GskWaveBatchFamily {
  uint32_t R, general;
  hipError_t (*launch)(const gsd::DevProblem* ds, uint32_t n, uint32_t wide, uint32_t lds, hipStream_t s);
  hipError_t (*set_lds)(uint32_t lds_total, uint32_t* dyn_min);
};
// ffd_sim_batch_r.hip: n problems at ds with blocks[i] workgroups of nt threads
// each; blocks_per_cu: resident workgroups at a dynamic LDS size (0: the query failed)
struct GskSimBatchFamily {
  uint32_t R, general;
  hipError_t (*launch)(const gsd::DevProblem* ds, const uint32_t* blocks, uint32_t n, uint32_t max_blocks, uint32_t nt,
                       uint32_t lds, uint32_t ov_epoch, hipStream_t s);
  hipError_t (*set_lds)(uint32_t lds_total, uint32_t* dyn_min);
  uint32_t (*blocks_per_cu)(uint32_t nt, uint32_t lds);
};
#define GSK_DECLARE_RT(r, t)                                                \
  extern "C" const GskWaveFamily* GSK_RT_NAME(gsk_ffdw, r, t)(void);        \
  extern "C" const GskWaveBatchFamily* GSK_RT_NAME(gsk_ffdwb, r, t)(void);  \
  extern "C" const GskSimBatchFamily* GSK_RT_NAME(gsk_ffdsb, r, t)(void);
GSK_FOR_EACH_RT(GSK_DECLARE_RT)
#undef GSK_DECLARE_RT
