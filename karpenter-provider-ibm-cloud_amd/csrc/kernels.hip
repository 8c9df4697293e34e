// kernels.hip — gfx950 (CDNA4, wave64) kernels of the provisioning solve.
//
//  K1/K2 feas_kernel   pod-variant x template x instance-type feasibility rows
//                      (one wave per (variant, template); lane = instance type;
//                      __ballot packs 64 ITs per word) + wave argmin of the
//                      cheapest compatible offering, key (price_rank<<32|name_rank)
//  K4    ffd_kernel    (ffd.hip) the sequential Scheduler.Solve queue loop as
//                      ONE persistent workgroup, or one workgroup per
//                      consolidation simulation
//  K3    trunc_kernel  per NodeClaim: OrderByPrice + Truncate(60)
//
// All integer/bitset work: no MFMA.  Semantics cited as <U> restate
// sigs.k8s.io/karpenter@v1.13.0 ("parity").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "devutil.hpp"
#include "kernel_api.hpp"
#include "layout.hpp"

using namespace gsd;

// K1/K2, K3 and the minValues settlement of simulations themselves (shared with
// the batched kernels of batch_kernels.hip)
#include "solve_kernels.hpp"

// ------------------------------------------------------------ host launchers
extern "C" hipError_t gsk_init_trunc(uint32_t trunc_lds_bytes) {
  return hipFuncSetAttribute((const void*)trunc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)trunc_lds_bytes);
}

template <uint32_t LP>
static void launch_feas_lp(const DevProblem* d, uint32_t static_mode, uint32_t w_lo, uint32_t w_hi, hipStream_t s) {
  const uint64_t pairs = (uint64_t)d->V * d->T;
  const uint64_t per_block = (BLOCK / 64) * (64 / LP);
  const uint32_t blocks = (uint32_t)((pairs + per_block - 1) / per_block);
  hipLaunchKernelGGL(feas_kernel<LP>, dim3(blocks), dim3(BLOCK), 0, s, *d, static_mode, w_lo, w_hi);
}

extern "C" hipError_t gsk_feas(const DevProblem* d, uint32_t static_mode, uint32_t w_lo, uint32_t w_hi,
                               hipStream_t s) {
  if (!d->V || !d->T) return hipSuccess;
  const uint64_t nc = (uint64_t)d->V * d->T * d->R;
  if (nc) hipLaunchKernelGGL(feas_cursor_kernel, dim3((uint32_t)((nc + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, *d);
  // lanes per pair: the row's word count rounded up to a power of two, at
  // most GS_K1_LPMAX (a lane then takes W / LP words; PP x W <= 256 keeps the
  // pairs' rows in the wave's LDS slice).  The kernel is a chain of dependent
  // loads per wave: more pairs per wave is fewer chains.  C5 (W = 32), same
  // session: LP 32 0.1268 ms, 16 0.1200, 8 0.1354 (profiles/r5/k1_lanes_ab.txt)
#ifndef GS_K1_LPMAX
#define GS_K1_LPMAX 16
#endif
  uint32_t W = d->W;
  if (GS_K1_LPMAX < 64 && W > GS_K1_LPMAX && W <= 32 && W * (64 / GS_K1_LPMAX) <= 256) W = GS_K1_LPMAX;
  if (W <= 1) launch_feas_lp<1>(d, static_mode, w_lo, w_hi, s);
  else if (W <= 2) launch_feas_lp<2>(d, static_mode, w_lo, w_hi, s);
  else if (W <= 4) launch_feas_lp<4>(d, static_mode, w_lo, w_hi, s);
  else if (W <= 8) launch_feas_lp<8>(d, static_mode, w_lo, w_hi, s);
  else if (W <= 16) launch_feas_lp<16>(d, static_mode, w_lo, w_hi, s);
  else if (W <= 32) launch_feas_lp<32>(d, static_mode, w_lo, w_hi, s);
  else launch_feas_lp<64>(d, static_mode, w_lo, w_hi, s);
  return hipGetLastError();
}

// <U> minValues (Strict) on the static matrix: a fresh NodeClaim whose
// options miss a template minimum is not addable, so its row is empty (no
// cheapest type, no offering).  One wave per (variant, template) pair whose
// template carries minValues; lane w holds words w, w + 64, ...
__global__ __launch_bounds__(BLOCK) void mv_rows_kernel(DevProblem d) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t pair = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6));
  if (pair >= d.V * d.T) return;  // wave-uniform
  const TmplRec& tr = d.tmpl[pair % d.T];
  if (!tr.mv_mask) return;
  uint64_t* row = d.rows + (size_t)pair * d.OW;
  bool ok = true;
  for (uint32_t mm = tr.mv_mask; mm && ok; mm &= mm - 1) {
    const uint32_t k = (uint32_t)__builtin_ctz(mm);
    uint32_t n = 0;
    if ((d.it_key_unique >> k) & 1) {
      for (uint32_t w = lane; w < d.W; w += 64) n += (uint32_t)__popcll(row[w]);
      n = wave_sum_u32(n);
    } else {
      const uint16_t* dv = d.it_dvid + (size_t)k * d.N;
      uint64_t sv[4] = {0, 0, 0, 0};
      for (uint32_t w = lane; w < d.W; w += 64)
        for (uint64_t m = row[w]; m; m &= m - 1) {
          const uint32_t x = dv[w * 64 + (uint32_t)__builtin_ctzll(m)];
#pragma unroll
          for (uint32_t q = 0; q < 4; q++) sv[q] |= (x >> 6) == q ? 1ull << (x & 63) : 0ull;
        }
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        for (int o = 32; o >= 1; o >>= 1) sv[q] |= shfl_xor_u64(sv[q], o);
        n += (uint32_t)__popcll(sv[q]);
      }
    }
    ok = n >= tr.mv[k];
  }
  if (ok) return;
  for (uint32_t w = lane; w < d.W; w += 64) row[w] = 0;
  if (lane == 0) {
    d.nfo[pair] = 0;
    d.cheapest[pair] = NONE;
    d.cheapest_key[pair] = 0x7FFFFFFFFFFFFFFFull;
  }
}

extern "C" hipError_t gsk_mv_rows(const DevProblem* d, hipStream_t s) {
  const uint64_t pairs = (uint64_t)d->V * d->T;
  if (!pairs) return hipSuccess;
  hipLaunchKernelGGL(mv_rows_kernel, dim3((uint32_t)((pairs + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, s, *d);
  return hipGetLastError();
}

// ==================================================== shard merge (multi-GPU)
// A sharded context's static matrix: shard k computed instance-type words
// [lo_k, hi_k) of every (variant, template) row on its own device.  One
// kernel on the parent's device gathers each word from the shard that owns
// it (peer loads over xGMI, or local memory when a device repeats), adds the
// per-shard offering counts and keeps the minimum OrderByPrice key (the
// cheapest offering's instance type is the key's name rank).  With RCCL the
// counts and keys were all-reduced already: shard 0's are final (K_red = 1).
extern "C" __global__ __launch_bounds__(BLOCK) void merge_shards_kernel(ShardMerge m) {
  const size_t stride = (size_t)gridDim.x * BLOCK, i0 = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t nw = m.we - m.wb;
  for (size_t i = i0; i < (size_t)m.VT * nw; i += stride) {
    const size_t vt = i / nw;
    const uint32_t w = m.wb + (uint32_t)(i % nw);
    uint32_t k = 0;
    while (k + 1 < m.K && w >= m.src[k].hi) k++;
    m.rows[vt * m.OW + w] = m.src[k].rows[vt * m.OW + w];
  }
  for (size_t vt = i0; vt < m.VT; vt += stride) {
    uint32_t n = 0;
    uint64_t key = 0x7FFFFFFFFFFFFFFFull;
    for (uint32_t k = 0; k < m.K_red; k++) {
      n += m.src[k].nfo[vt];
      const uint64_t x = m.src[k].key[vt];
      key = x < key ? x : key;
    }
    m.nfo[vt] = n;
    m.key[vt] = key;
    m.cheapest[vt] = key == 0x7FFFFFFFFFFFFFFFull ? NONE : m.rank_to_it[(uint32_t)key];
  }
}

extern "C" hipError_t gsk_merge_shards(const ShardMerge* m, hipStream_t s) {
  const size_t work = (size_t)m->VT * (m->we - m->wb > 0 ? m->we - m->wb : 1);
  const uint32_t grid = (uint32_t)std::min<size_t>((work + BLOCK - 1) / BLOCK, 8192);
  hipLaunchKernelGGL(merge_shards_kernel, dim3(grid ? grid : 1), dim3(BLOCK), 0, s, *m);
  return hipGetLastError();
}

// simulations with minValues (any_mv): every NodeClaim arena slot, then the
// per-simulation settlement; otherwise one block per simulation / NodeClaim
extern "C" hipError_t gsk_trunc(const DevProblem* d, uint32_t lds_bytes, uint32_t n_slots, hipStream_t s) {
  if (d->n_sims && d->any_mv) {
    if (!n_slots) return hipSuccess;
    hipLaunchKernelGGL(trunc_kernel, dim3(n_slots), dim3(BLOCK), lds_bytes, s, *d, 1u, 0u);
    hipLaunchKernelGGL(sim_fix_kernel, dim3((d->n_sims + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, *d);
    return hipGetLastError();
  }
  const uint32_t grid = d->n_sims ? d->n_sims : d->claim_cap;
  if (!grid) return hipSuccess;
  hipLaunchKernelGGL(trunc_kernel, dim3(grid), dim3(BLOCK), lds_bytes, s, *d, 0u, 0u);
  return hipGetLastError();
}

// every NodeClaim of one simulation (arena slots slot0 .. slot0 + n_slots) into
// slots 0.. of d->slot_its / slot_nits / slot_drop (gs_consolidation_results;
// d->n_sims - 1 is that simulation)
extern "C" hipError_t gsk_trunc_slots(const DevProblem* d, uint32_t lds_bytes, uint32_t slot0, uint32_t n_slots,
                                      hipStream_t s) {
  if (!n_slots) return hipSuccess;
  hipLaunchKernelGGL(trunc_kernel, dim3(n_slots), dim3(BLOCK), lds_bytes, s, *d, 1u, slot0);
  return hipGetLastError();
}
