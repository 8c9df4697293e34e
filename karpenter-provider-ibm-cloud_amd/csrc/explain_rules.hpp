// explain_rules.hpp — gs_explain's one rule: from what is known of a (pod
// variant, NodeClaim template) pair to the cause code, shared by
// explain_kernel (explain.hip, which packs the code into the pair's word),
// the host side of gs_explain (the NodePools without a template) and the
// host-only program tools/explain_rules_harness.cpp, which walks the same text
// on the CPU.
//
// <U> restated from memory of sigs.k8s.io/karpenter v1.13: the order of the
// checks for one NodeClaimTemplate in Scheduler.add -> NodeClaim.CanAdd
// (Taints.ToleratesPod, Requirements.Compatible) ->
// filterInstanceTypesByRequirements, and the chain of
// InstanceTypeFilterError.Error() over its seven booleans.  The first code
// that applies wins.
#pragma once
#include <stdint.h>

// g++ builds (sanitizers, the host program) see the functions without the HIP attributes
#ifdef __HIPCC__
#define GSX_FN __host__ __device__
#else
#define GSX_FN
#endif

namespace gsx {

// gs_explain_result.cause (GS_WHY_*, include/gpusched.h: same values)
enum : uint32_t {
  WHY_STATE = 0,
  WHY_NO_OPTIONS = 1,
  WHY_LIMITS = 2,
  WHY_TAINTS = 3,
  WHY_INCOMPATIBLE = 4,
  WHY_MIN_VALUES = 5,
  WHY_IT_NONE = 6,
  WHY_IT_REQ_OR_FITS = 7,
  WHY_IT_REQ_OR_OFFERING = 8,
  WHY_IT_FITS_OR_OFFERING = 9,
  WHY_IT_REQUIREMENTS = 10,
  WHY_IT_RESOURCES = 11,
  WHY_IT_OFFERING = 12,
  WHY_IT_REQ_FITS_NO_OFFERING = 13,
  WHY_IT_FITS_OFFERING_NO_REQ = 14,
  WHY_IT_REQ_OFFERING_NO_FITS = 15,
  WHY_IT_TUPLE = 16,
  WHY_COUNT = 17
};

// gs_explain_result.met (GS_MET_*): upstream's seven booleans
enum : uint32_t {
  MET_REQUIREMENTS = 1u << 0,
  MET_FITS = 1u << 1,
  MET_OFFERING = 1u << 2,
  MET_REQ_FITS_ONLY = 1u << 3,      // requirements and resources, no offering
  MET_REQ_OFFERING_ONLY = 1u << 4,  // requirements and offering, not the resources
  MET_FITS_OFFERING_ONLY = 1u << 5, // resources and offering, not the requirements
  MET_ALL = 1u << 6,
  MET_MASK = 0x7Fu
};

// what is decided before the instance types are looked at, and the minValues
// verdict on the options that met all three
enum : uint32_t {
  PRE_NO_OPTIONS = 1u << 0,    // the NodePool kept no option at NewScheduler (no template)
  PRE_LIMITS = 1u << 1,        // options, but none within the NodePool's limits as given
  PRE_TAINTS = 1u << 2,        // a taint of the NodePool is not tolerated
  PRE_INCOMPATIBLE = 1u << 3,  // Requirements.Compatible(pod, AllowUndefinedWellKnownLabels) fails
  PRE_MIN_VALUES = 1u << 4,    // the options that met all three miss a template minValues
  PRE_MASK = 0x1Fu
};

GSX_FN inline __attribute__((always_inline)) uint32_t cause_of(uint32_t met, uint32_t pre) {
  if (pre & PRE_NO_OPTIONS) return WHY_NO_OPTIONS;
  if (pre & PRE_LIMITS) return WHY_LIMITS;
  if (pre & PRE_TAINTS) return WHY_TAINTS;
  if (pre & PRE_INCOMPATIBLE) return WHY_INCOMPATIBLE;
  if (met & MET_ALL) return (pre & PRE_MIN_VALUES) ? WHY_MIN_VALUES : WHY_STATE;
  const bool r = met & MET_REQUIREMENTS, f = met & MET_FITS, o = met & MET_OFFERING;
  if (!r && !f && !o) return WHY_IT_NONE;
  if (!r && !f) return WHY_IT_REQ_OR_FITS;
  if (!r && !o) return WHY_IT_REQ_OR_OFFERING;
  if (!f && !o) return WHY_IT_FITS_OR_OFFERING;
  if (!r) return WHY_IT_REQUIREMENTS;
  if (!f) return WHY_IT_RESOURCES;
  if (!o) return WHY_IT_OFFERING;
  if (met & MET_REQ_FITS_ONLY) return WHY_IT_REQ_FITS_NO_OFFERING;
  if (met & MET_FITS_OFFERING_ONLY) return WHY_IT_FITS_OFFERING_NO_REQ;
  if (met & MET_REQ_OFFERING_ONLY) return WHY_IT_REQ_OFFERING_NO_FITS;
  return WHY_IT_TUPLE;
}

// `met` as reported: 0 where the cause is decided before the instance types
GSX_FN inline __attribute__((always_inline)) uint32_t met_reported(uint32_t met, uint32_t pre) {
  return (pre & (PRE_NO_OPTIONS | PRE_LIMITS | PRE_TAINTS | PRE_INCOMPATIBLE)) ? 0u : (met & MET_MASK);
}

// one pair's packed word (explain_kernel writes it, the host unpacks it):
//   bits 0..6   met, as reported
//   bits 8..12  cause
//   bits 16..22 for WHY_TAINTS: 1 + the position, in the template's ordered
//               taint-class list, of the first untolerated class
GSX_FN inline __attribute__((always_inline)) uint32_t pack(uint32_t met, uint32_t pre, uint32_t taint_pos) {
  const uint32_t cause = cause_of(met, pre);
  return met_reported(met, pre) | (cause << 8) | (cause == WHY_TAINTS ? ((taint_pos + 1) & 0x7Fu) << 16 : 0u);
}
GSX_FN inline __attribute__((always_inline)) uint32_t packed_met(uint32_t w) { return w & MET_MASK; }
GSX_FN inline __attribute__((always_inline)) uint32_t packed_cause(uint32_t w) { return (w >> 8) & 0x1Fu; }
// NONE-like 0xFFFFFFFF when no position is packed
GSX_FN inline __attribute__((always_inline)) uint32_t packed_taint_pos(uint32_t w) { return ((w >> 16) & 0x7Fu) - 1u; }

}  // namespace gsx
