// filter_rules.hpp — the Create re-filter's HBM records and its rule for one
// (claim, instance type) pair, shared by the two kernels (filter.hip), the
// host reducer (filter_encode.cpp) and the host-only harness
// (tools/encode_harness.cpp -f), which evaluates the same text on the CPU.
//
// Every requirement list is reduced on the host to one FReq per (normalised)
// key, key-sorted within a list: complement flag, Gt/Lt bounds and a sorted
// run of dense value ids.  Requirements.Compatible for a pair merges the two
// key-sorted lists.
#pragma once
#include <stddef.h>
#include <stdint.h>

// g++ builds (sanitizers, the harness) see the functions without the HIP attributes
#ifdef __HIPCC__
#define GSF_FN __host__ __device__
#else
#define GSF_FN
#endif

namespace gsf {

enum : uint32_t { F_COMP = 1, F_GT = 2, F_LT = 4, F_WK = 8 };

struct FReq {
  uint32_t key, flags, vb, vn;
  int64_t gt, lt;
};
struct FList {
  uint32_t b, n;
};
struct FIt {
  FList reqs;
  uint32_t ob, on;
  uint32_t alloc_neg, pad;
};
struct FOff {
  FList reqs;
  uint32_t available, spot;
};
struct FQty {
  uint32_t r, pad;
  int64_t v;
};
struct FQuery {
  FList reqs;
  uint32_t qb, qn;
  uint32_t spot;    // the claim's capacity-type requirement allows spot
  uint32_t vb, vn;  // the list's values: vals[vb, vb + vn), in requirement order
  uint32_t pad;
};
static_assert(sizeof(FReq) == 32 && sizeof(FIt) == 24 && sizeof(FOff) == 16 && sizeof(FQty) == 16 &&
                  sizeof(FQuery) == 32,
              "filter layout");

// claim_select_kernel's claim staging budget (LDS per workgroup): a claim
// whose reduced list has at most kSelLdsReqs keys and kSelLdsVals values in
// all is copied to LDS once (1 KiB + 4 KiB); a longer one is read from HBM
constexpr uint32_t kSelLdsReqs = 32, kSelLdsVals = 1024;
GSF_FN inline bool sel_fits_lds(uint32_t n_reqs, uint32_t n_vals) {
  return n_reqs <= kSelLdsReqs && n_vals <= kSelLdsVals;
}

// one claim's outcome (claim_select_kernel): 16 B
struct FRec {
  uint32_t n_compatible;
  int32_t selected;
  uint32_t capacity_type, zero;
};
static_assert(sizeof(FRec) == 16, "filter record");

GSF_FN inline __attribute__((always_inline)) bool exempt(const FReq& q) {
  // Operator() in {NotIn, DoesNotExist}
  return (q.flags & F_COMP) ? q.vn != 0 : q.vn == 0;
}

GSF_FN inline __attribute__((always_inline)) bool contains(const uint32_t* v, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t m = (lo + hi) >> 1;
    if (v[m] < x) lo = m + 1;
    else hi = m;
  }
  return lo < n && v[lo] == x;
}

// <U> Requirement.Intersection(a, b).Len() == 0; av / bv: the vals array each
// side's vb indexes (D: where a value id's parsed integer lives)
template <class D>
GSF_FN bool len_zero(const D& d, const FReq& a, const uint32_t* av, const FReq& b, const uint32_t* bv) {
  const bool hg = (a.flags | b.flags) & F_GT, hl = (a.flags | b.flags) & F_LT;
  int64_t gt = (a.flags & F_GT) ? a.gt : b.gt;
  if ((a.flags & F_GT) && (b.flags & F_GT)) gt = a.gt > b.gt ? a.gt : b.gt;
  int64_t lt = (a.flags & F_LT) ? a.lt : b.lt;
  if ((a.flags & F_LT) && (b.flags & F_LT)) lt = a.lt < b.lt ? a.lt : b.lt;
  if (hg && hl && gt >= lt) return true;  // DoesNotExist
  const bool ac = a.flags & F_COMP, bc = b.flags & F_COMP;
  if (ac && bc) return false;  // MaxInt64 - |union| > 0
  // walk the concrete side (the smaller one when both are concrete)
  // (selected field by field: pointers to a and b would put both in scratch)
  const bool swap = ac || (!bc && b.vn < a.vn);
  const uint32_t* sv = (swap ? bv : av) + (swap ? b.vb : a.vb);
  const uint32_t* ov = (swap ? av : bv) + (swap ? a.vb : b.vb);
  const uint32_t sn = swap ? b.vn : a.vn, on = swap ? a.vn : b.vn;
  const bool want = !((swap ? a.flags : b.flags) & F_COMP);  // concrete other: intersection; complement: difference
  for (uint32_t i = 0; i < sn; i++) {
    const uint32_t v = sv[i];
    if (contains(ov, on, v) != want) continue;
    if (hg || hl) {
      if (!d.vok_at(v)) continue;
      const int64_t x = d.vint_at(v);
      if ((hg && gt >= x) || (hl && lt <= x)) continue;
    }
    return false;
  }
  return true;
}

// <U> Requirements.Compatible(incoming, AllowUndefinedWellKnownLabels):
// incoming keys the existing list lacks must be well known or NotIn /
// DoesNotExist; shared keys must intersect unless both are NotIn/DoesNotExist
template <class D>
GSF_FN bool compatible(const D& d, const FReq* ex, uint32_t en, const uint32_t* exv, const FReq* in, uint32_t inn,
                       const uint32_t* inv) {
  uint32_t i = 0;
  for (uint32_t j = 0; j < inn; j++) {
    const FReq b = in[j];
    while (i < en && ex[i].key < b.key) i++;
    if (i < en && ex[i].key == b.key) {
      const FReq a = ex[i];
      if (len_zero(d, a, exv, b, inv) && !(exempt(a) && exempt(b))) return false;
    } else if (!(b.flags & F_WK) && !exempt(b)) {
      return false;
    }
  }
  return true;
}

// pair_verdict's bits
enum : uint32_t {
  P_REQS = 1,    // the claim's requirements are Compatible with the type's
  P_CREATE = 2,  // ... and the requests fit and some available offering is compatible: Create keeps the type
  P_SPOT = 4,    // ... and that offering walk reached a spot one
};

// The rule for claim Q (list qr, its values in qv) against instance type `it`
// of d (lists in cr, their values in cv): Compatible, then Fits, then the walk
// over the available offerings, which stops at the first spot one.  D supplies
// its, offs, alloc ([N][R]), qty, R, vok_at and vint_at.
template <class D>
GSF_FN inline __attribute__((always_inline)) uint32_t pair_verdict(const D& d, const FQuery& Q, const FReq* qr,
                                                                   const uint32_t* qv, const FReq* cr,
                                                                   const uint32_t* cv, uint32_t it) {
  const FIt I = d.its[it];
  const bool ok_req = compatible(d, qr, Q.reqs.n, qv, cr + I.reqs.b, I.reqs.n, cv);
  bool fits = !I.alloc_neg;
  for (uint32_t k = 0; fits && k < Q.qn; k++) {
    const FQty x = d.qty[Q.qb + k];
    // a resource no capacity list names: Allocatable() reads 0
    fits = x.v <= (x.r < d.R ? d.alloc[(size_t)it * d.R + x.r] : 0);
  }
  bool any = false, spot = false;
  for (uint32_t o = 0; ok_req && fits && o < I.on; o++) {
    const FOff f = d.offs[I.ob + o];
    if (!f.available || !compatible(d, qr, Q.reqs.n, qv, cr + f.reqs.b, f.reqs.n, cv)) continue;
    any = true;
    if (f.spot) {
      spot = true;
      break;
    }
  }
  const bool ok_create = ok_req && fits && any;
  return (ok_req ? P_REQS : 0) | (ok_create ? P_CREATE : 0) | (spot && ok_create ? P_SPOT : 0);
}

}  // namespace gsf
