// rank_rules.hpp — the autoplacement ranking's two rules for one instance
// type, shared by gs_rank_instance_types (rank.hip), the resident-catalog form
// gs_rank_prepare / _run (rank_batch.hip) and the host-only program
// tools/rank_rules_host.cpp, which evaluates the same text on the CPU.
//
//   keep():  IBMInstanceTypeProvider.FilterInstanceTypes' four filters
//            (pkg/providers/common/instancetype/instancetype.go:319-344)
//   score(): calculateInstanceTypeScore (:90-110), float64
//
// Both take plain values.  The !(x < y) forms are deliberate: they carry the
// reference's outcomes for NaN and +-inf operands (a NaN max_price switches
// the filter off, an infinite cost efficiency compares as Go's does).
#pragma once
#include <stdint.h>

// g++ builds (sanitizers, the host program) see the functions without the HIP attributes
#ifdef __HIPCC__
#define GSR_FN __host__ __device__
#else
#define GSR_FN
#endif

namespace gsr {

constexpr uint32_t kArchAny = 0xFFFFFFFFu;  // GS_ARCH_ANY

// Capacity.Cpu().Value() and Memory().ScaledValue(Giga) round up
GSR_FN inline __attribute__((always_inline)) int64_t cpu_cores(int64_t cpu_milli) { return (cpu_milli + 999) / 1000; }
GSR_FN inline __attribute__((always_inline)) int64_t memory_gb(int64_t memory_bytes) {
  return (memory_bytes + 999999999) / 1000000000;
}

// want_arch == kArchAny, min_cpu <= 0, min_memory_gb <= 0 and a max_price
// that is not > 0 (NaN included) each switch their filter off
GSR_FN inline __attribute__((always_inline)) bool keep(int64_t cpu_milli, int64_t memory_bytes, double price,
                                                       uint32_t arch, uint32_t want_arch, int64_t min_cpu,
                                                       int64_t min_memory_gb, double max_price) {
  const int64_t cpu = cpu_cores(cpu_milli);
  return (want_arch == kArchAny || arch == want_arch) && (min_cpu <= 0 || cpu >= min_cpu) &&
         (min_memory_gb <= 0 || !((double)memory_bytes / 1073741824.0 < (double)min_memory_gb)) &&
         (!(max_price > 0) || !(price > max_price));
}

GSR_FN inline __attribute__((always_inline)) double score(int64_t cpu_milli, int64_t memory_bytes, double price) {
  const int64_t cpu = cpu_cores(cpu_milli);
  const int64_t mem_gb = memory_gb(memory_bytes);
  if (price <= 0) return (double)cpu + (double)mem_gb;
  const double ce = price / (double)cpu;
  const double me = price / (double)mem_gb;
  return (ce + me) / 2;
}

}  // namespace gsr
