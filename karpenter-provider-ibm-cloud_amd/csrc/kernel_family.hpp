// kernel_family.hpp — the (R, TOPO) families of the Solve kernels, listed once.
// Every Solve kernel is instantiated per resource count R = 1..8 and per
// variant (0: plain, 1: general, layout.hpp general_variant).  A unit that
// holds a family's instantiations describes it in one record that starts with
// the two uint32_t members R and general; a dispatcher builds a table of the
// sixteen records with GSK_FOR_EACH_RT and finds its entry with gsk_family, so
// launch, LDS attribute and occupancy of a problem come from the same record.
// (Records and tables are statics of host functions: a const object at
// namespace scope would be emitted into the device code as well.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// M(R, x) for every R, and M(R, TOPO) for the sixteen pairs in (R, TOPO) order
#define GSK_FOR_EACH_R(M, x) M(1, x) M(2, x) M(3, x) M(4, x) M(5, x) M(6, x) M(7, x) M(8, x)
#define GSK_RT_PAIR(r, M) M(r, 0) M(r, 1)
#define GSK_FOR_EACH_RT(M) GSK_FOR_EACH_R(GSK_RT_PAIR, M)

// stem_r<R>_t<T>: the exported function of one family, which returns its record
// (macro arguments expand first)
#define GSK_RT_NAME2(stem, r, t) stem##_r##r##_t##t
#define GSK_RT_NAME(stem, r, t) GSK_RT_NAME2(stem, r, t)

// the table's record of (R, general); nullptr: R outside 1..8
template <class F, size_t N>
inline const F* gsk_family(const F* const (&table)[N], uint32_t R, bool general) {
  for (const F* f : table)
    if (f->R == R && (f->general != 0) == general) return f;
  return nullptr;
}

// set_lds of every family of the table (the last error, if any); *dyn_max: the
// smallest dynamic LDS size an instantiation was left with
template <class F, size_t N>
inline hipError_t gsk_set_lds(const F* const (&table)[N], uint32_t lds_total, uint32_t* dyn_max) {
  hipError_t e = hipSuccess;
  uint32_t dmin = 0;
  for (const F* f : table)
    if (hipError_t x = f->set_lds(lds_total, &dmin); x != hipSuccess) e = x;
  *dyn_max = dmin;
  return e;
}

// Let kernel `fn` use all the LDS its static footprint leaves free of
// lds_total; *dyn_min keeps the smallest such size over the calls (0: none yet)
inline hipError_t set_max_dyn_lds(const void* fn, uint32_t lds_total, uint32_t* dyn_min) {
  hipFuncAttributes a;
  const hipError_t e = hipFuncGetAttributes(&a, fn);
  if (e != hipSuccess) return e;
  const uint32_t dyn = lds_total > a.sharedSizeBytes ? lds_total - (uint32_t)a.sharedSizeBytes : 0;
  if (!*dyn_min || dyn < *dyn_min) *dyn_min = dyn;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
}
