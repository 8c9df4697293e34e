// init_kernel.hpp — the Solve's state reset, compiled in its single-problem
// form by ffd_wave.hip and in its batched form by batch_kernels.hip
// (kernel_problem.hpp).
#pragma once
#include "kernel_problem.hpp"

// Grid-wide reset of the Solve's working state (queue, per-pod counters,
// NodePool remaining limits, existing-node copies, hostname counts): the
// single-wave kernel starts from it.
extern "C" __global__ __launch_bounds__(256) void GS_KNAME(ffd_init_kernel)(GS_KPROBLEM_ARG) {
  GS_KPROBLEM
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = i0; i < d.P; i += stride) {
    d.queue[i] = d.queue0[i];
    d.last_epoch[i] = 0;
    d.last_len[i] = 0;
    d.cur_var[i] = d.var_begin[i];
  }
  for (uint32_t i = i0; i < d.T * d.R; i += stride) d.t_rem[i] = d.tmpl[i / d.R].limits[i % d.R];
  for (uint32_t i = i0; i < d.NN; i += stride) d.nodes[i] = d.nodes0[i];
  for (uint32_t i = i0; i < d.NN * d.F; i += stride) d.n_fk[i] = d.n_fk0[i];
  for (uint32_t i = i0; i < d.TGH * d.NN; i += stride) d.hn[i] = d.hn0[i];
  if (d.any_vol)
    for (uint32_t i = i0; i < d.NN; i += stride) d.n_vol[i] = d.n_vol0[i];
}
