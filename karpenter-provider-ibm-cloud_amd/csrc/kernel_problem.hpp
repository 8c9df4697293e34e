// kernel_problem.hpp — how a Solve-path grid kernel receives its problem.  The
// kernels of solve_kernels.hpp, queue_kernels.hpp and init_kernel.hpp are
// written once: a unit that defines GS_BATCH_KERNELS (batch_kernels.hip)
// compiles their batched form, <name>_batch(const DevProblem* ds, ...), where
// the problem is element blockIdx.y of a device array and gridDim.x is sized
// for the largest problem of the launch; every other unit compiles the
// single-problem form, <name>(DevProblem d, ...), exactly as written before
// the batch existed.
#pragma once
#ifdef GS_BATCH_KERNELS
#define GS_KNAME(name) name##_batch
#define GS_KPROBLEM_ARG const DevProblem* __restrict__ ds
// the index is uniform over the workgroup: the fields arrive by scalar loads
#define GS_KPROBLEM const DevProblem& d = ds[blockIdx.y];
// a block past its own problem's extent leaves before any barrier or LDS use
#define GS_KPROBLEM_EXIT(cond) \
  if (cond) return;
#else
#define GS_KNAME(name) name
#define GS_KPROBLEM_ARG DevProblem d
#define GS_KPROBLEM
#define GS_KPROBLEM_EXIT(cond)
#endif
