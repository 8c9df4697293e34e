// queue_kernels.hpp — the first-pass queue record kernels, compiled in their
// single-problem form by ffd.hip and in their batched form by
// batch_kernels.hip (kernel_problem.hpp).
#pragma once
#include "kernel_problem.hpp"

// ================================================ first-pass queue records
// The Solve's first pass pops pods in queue0 order with their first variant:
// the records are gathered into queue order here, on the device, from the
// arrays the upload already holds (one thread per queue position; HBM-bound,
// ~0.2 KB per pod), instead of being built on the host and copied a second
// time over PCIe.  qcodes: qcode_floor / qcode_ceil of resources 0..3 packed
// 16 bits each, the wave Solve's SWAR operands.
__global__ __launch_bounds__(256) void GS_KNAME(queue_records_kernel)(GS_KPROBLEM_ARG) {
  GS_KPROBLEM
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= d.P) return;
  const uint32_t p = d.queue0[k];
  const uint4* src = (const uint4*)(d.vars + d.var_begin[p]);
  uint4* dst = (uint4*)(const_cast<VarRec*>(d.qvars) + k);
#pragma unroll
  for (uint32_t q = 0; q < sizeof(VarRec) / sizeof(uint4); q++) dst[q] = src[q];
  int64_t* qr = const_cast<int64_t*>(d.qreqs) + (size_t)k * d.R;
  uint64_t fl = 0, ce = 0;
  for (uint32_t r = 0; r < d.R; r++) {
    const int64_t v = d.pod_req[(size_t)p * d.R + r];
    qr[r] = v;
    if (r < 4) {
      fl |= (uint64_t)qcode_floor(v) << (16 * r);
      ce |= (uint64_t)qcode_ceil(v) << (16 * r);
    }
  }
  uint4 c;
  c.x = (uint32_t)fl;
  c.y = (uint32_t)(fl >> 32);
  c.z = (uint32_t)ce;
  c.w = (uint32_t)(ce >> 32);
  ((uint4*)const_cast<uint32_t*>(d.qcodes))[k] = c;
}

// qrun[k]: how many records from k on (at most the ring's 16) equal record k
// in every dword the wave Solve's run mode compares (all but the pod and the
// variant index): the run batch read it from the ring instead of comparing
// 16 staged records.  The batch was rejected and removed; this
// launch, qrun and the ring lane that carries it are still to go.  One
// comparison per adjacent pair (same[x]: record x equals record x + 1) into
// LDS, block range plus a 15-entry halo, then a scan of at most 15 bits
__device__ __forceinline__ bool queue_record_same(const DevProblem& d, uint32_t a, uint32_t b) {
  const uint4* va = (const uint4*)(d.qvars + a);
  const uint4* vb = (const uint4*)(d.qvars + b);
  bool same = true;
#pragma unroll
  for (uint32_t q = 0; q < sizeof(VarRec) / 16; q++) {
    const uint4 x = va[q], y = vb[q];
    // dword 0 (pod) and the last dword (variant index) may differ
    same = same && (q == 0 || x.x == y.x) && x.y == y.y && x.z == y.z && (q == sizeof(VarRec) / 16 - 1 || x.w == y.w);
  }
  for (uint32_t r = 0; r < d.R; r++) same = same && d.qreqs[(size_t)a * d.R + r] == d.qreqs[(size_t)b * d.R + r];
  return same;  // the codes follow from the requests
}
__global__ __launch_bounds__(256) void GS_KNAME(queue_runs_kernel)(GS_KPROBLEM_ARG) {
  GS_KPROBLEM
  GS_KPROBLEM_EXIT(blockIdx.x * 256 >= d.P)
  __shared__ uint8_t s_same[256 + 16];
  const uint32_t b0 = blockIdx.x * 256;
  for (uint32_t t = threadIdx.x; t < 256 + 16; t += 256) {
    const uint32_t x = b0 + t;
    s_same[t] = x + 1 < d.P && queue_record_same(d, x, x + 1);
  }
  __syncthreads();
  const uint32_t k = b0 + threadIdx.x;
  if (k >= d.P) return;
  uint32_t n = 1;
  while (n < 16 && s_same[threadIdx.x + n - 1]) n++;
  const_cast<uint32_t*>(d.qrun)[k] = n;
}
