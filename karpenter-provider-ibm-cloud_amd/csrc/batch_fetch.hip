// batch_fetch.hip — gs_batch_fetch_all's device pass: the records gs_fetch
// copies back per slot (the control block, the add log, the NodeClaim headers,
// their OrderByPrice rows and the pods left in the queue), packed for every
// batched slot into one staging buffer (batch_fetch_layout.hpp).  The kernels
// read the device array of problems the run used and are not templated on
// (R, TOPO, WIDE): two launches cover every slot of every group.
//
//  sizes  one workgroup: each slot's sizes from its control block, clamped
//         against the slot's own bounds (a slot over one is flagged and gets no
//         payload), an exclusive prefix sum in device array order, a FetchHead
//         per slot and the total in the FetchTop.  No atomic cursor: the layout
//         is the same from run to run.
//  copy   workgroup (chunk, slot): the slot's payload in 16-byte units, grid
//         stride over the chunks.  A total over the staging capacity copies
//         nothing (the host grows the buffer and launches again).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_fetch_layout.hpp"
#include "kernel_api.hpp"
#include "layout.hpp"

using namespace gsd;
using namespace gsbf;

static_assert(sizeof(LogRec) == kLogRecBytes, "LogRec size");
static_assert(sizeof(ClaimRec) == kClaimRecBytes, "ClaimRec size");
static_assert(kItsRowBytes % 16 == 0, "an option row is whole 16-byte units");

// ------------------------------------------------------------------- sizes
// gridDim = 1.  Slots are taken 256 at a time; within a chunk the prefix is a
// wave scan and a scan over the four waves' sums, as cons_settle_kernel_batch's.
extern "C" __global__ __launch_bounds__(256) void fetch_sizes_kernel_batch(const DevProblem* __restrict__ ds, uint32_t n,
                                                                           FetchTop* __restrict__ top,
                                                                           FetchHead* __restrict__ heads) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  __shared__ unsigned long long s_wave[4];
  unsigned long long run = 0;  // payload bytes of the slots before this chunk (uniform)
  for (uint32_t k0 = 0; k0 < n; k0 += 256) {
    const uint32_t k = k0 + tid;
    FetchHead h{};
    if (k < n) {
      const DevProblem& d = ds[k];
      const Ctrl& c = *d.ctrl;
      h.status = c.status;
      h.n_claims = c.n_claims;
      h.n_log = c.n_log;
      h.qhead = c.qhead;
      h.qlen = c.qlen;
      h.pops = c.pops;
      h.generic_sorts = c.generic_sorts;
      h.fast_sorts = c.fast_sorts;
      h.cand_evals = c.cand_evals;
      h.cand_full = c.cand_full;
      h.node_prefix = c.node_prefix;
      h.claim_prefix = c.claim_prefix;
      h.t_sort = c.t_sort;
      h.t_scan = c.t_scan;
      h.t_tmpl = c.t_tmpl;
      if (h.n_log > d.P || h.n_claims > d.claim_cap || h.qlen > d.P)
        h.flags = FH_CORRUPT;
      else if (h.status == 0)
        h.bytes = payload_bytes(h.n_log, h.n_claims, h.qlen);
    }
    unsigned long long incl = h.bytes;
    for (uint32_t s = 1; s < 64; s <<= 1) {
      const unsigned long long up = __shfl_up(incl, s, 64);
      if (lane >= s) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (uint32_t w = 0; w < 4; w++) {
      before += w < wave ? s_wave[w] : 0ull;
      total += s_wave[w];
    }
    __syncthreads();  // s_wave is rewritten by the next chunk
    if (k < n) {
      h.off = run + before + incl - h.bytes;
      heads[k] = h;
    }
    run += total;
  }
  if (tid == 0) {
    FetchTop t{};
    t.total = run;
    t.n = n;
    *top = t;
  }
}

// -------------------------------------------------------------------- copy
// gridDim = (chunks, n).  cap: payload bytes the staging buffer holds.  The
// early exits are uniform over the workgroup; the kernel has no barrier and no
// LDS.  Every source array starts a 256-byte aligned sub-buffer of the slot's
// arena and every payload region is 16-byte aligned, so the log, the headers
// and the option rows move as uint4; the NodeClaims' option counts and the
// queue are gathered four to a unit (zero past their end).
extern "C" __global__ __launch_bounds__(256) void fetch_copy_kernel_batch(const DevProblem* __restrict__ ds,
                                                                          const FetchTop* __restrict__ top,
                                                                          const FetchHead* __restrict__ heads,
                                                                          uint4* __restrict__ payload, uint64_t cap) {
  if (top->total > cap) return;
  const FetchHead& h = heads[blockIdx.y];
  if (!h.bytes || (h.flags & FH_CORRUPT) || h.off + h.bytes > cap) return;
  const DevProblem& d = ds[blockIdx.y];
  const uint32_t M = h.n_claims, qlen = h.qlen, P = d.P;
  const FetchRegions r = regions(h.n_log, M, qlen);
  const uint64_t u_rec = r.rec / 16, u_its = r.its / 16, u_nits = r.nits / 16, u_unp = r.unplaced / 16, u_end = r.end / 16;
  const uint4* log = (const uint4*)d.log;
  const uint4* rec = (const uint4*)d.c_rec;
  const uint4* its = (const uint4*)d.c_its;
  const uint32_t* nits = d.c_nits;
  const uint32_t* queue = d.queue;
  const uint32_t qh = P ? h.qhead % P : 0u;
  uint4* dst = payload + h.off / 16;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u < u_end; u += (uint64_t)gridDim.x * 256) {
    uint4 v;
    if (u < u_rec) {
      v = log[u];
    } else if (u < u_its) {
      v = rec[u - u_rec];
    } else if (u < u_nits) {
      v = its[u - u_its];
    } else if (u < u_unp) {
      const uint32_t j = (uint32_t)(u - u_nits) * 4u;
      v.x = j < M ? nits[j] : 0u;
      v.y = j + 1 < M ? nits[j + 1] : 0u;
      v.z = j + 2 < M ? nits[j + 2] : 0u;
      v.w = j + 3 < M ? nits[j + 3] : 0u;
    } else {
      // qlen <= P and qh < P: qh + i < 2P fits 64 bits, one conditional subtract
      const uint32_t i = (uint32_t)(u - u_unp) * 4u;
      auto at = [&](uint32_t x) -> uint32_t {
        if (x >= qlen) return 0u;
        uint64_t q = (uint64_t)qh + x;
        if (q >= P) q -= P;
        return queue[q];
      };
      v.x = at(i);
      v.y = at(i + 1);
      v.z = at(i + 2);
      v.w = at(i + 3);
    }
    dst[u] = v;
  }
}

// n slots (the whole device array): two launches.  max_pods: the largest slot's
// pods, which sizes the chunk count (the copy is a grid-stride loop, so any
// count is correct).
extern "C" hipError_t gsk_fetch_gather_batch(const DevProblem* ds, uint32_t n, uint32_t max_pods, void* staging,
                                             uint64_t payload_cap, hipStream_t s) {
  if (!n || n > kMaxSlots) return hipErrorInvalidValue;
  char* base = (char*)staging;
  FetchTop* top = (FetchTop*)base;
  FetchHead* heads = (FetchHead*)(base + kTopBytes);
  uint4* payload = (uint4*)(base + payload_base(n));
  uint32_t chunks = (max_pods + 255u) / 256u;
  chunks = chunks < 1u ? 1u : chunks > 16u ? 16u : chunks;
  hipLaunchKernelGGL(fetch_sizes_kernel_batch, dim3(1), dim3(256), 0, s, ds, n, top, heads);
  hipLaunchKernelGGL(fetch_copy_kernel_batch, dim3(chunks, n), dim3(256), 0, s, ds, (const FetchTop*)top,
                     (const FetchHead*)heads, payload, payload_cap);
  return hipGetLastError();
}
