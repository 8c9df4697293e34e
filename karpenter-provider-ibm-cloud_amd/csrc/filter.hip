// filter.hip — launch-time re-filter of emitted NodeClaims (gs_create_filter
// and its prepared form gs_create_filter_prepare / _run / _set_available):
// CloudProvider.Create's instance-type filter (reference
// pkg/cloudprovider/cloudprovider.go:322-346), GetInstanceTypes' NodePool
// filter (:574-577), the instance provider's instanceTypes[0] pick
// (pkg/providers/vpc/instance/provider.go:215-221) and ResolveCapacityType
// (pkg/providers/common/capacitytype/capacitytype.go:27-42), for a batch of
// NodeClaims in one device pass.
//
// Unlike the Solve encoder (encode.cpp), which folds requirements into
// per-key vocabulary bitsets under the restrictions the FFD kernels need,
// this path keeps the general <U> scheduling.Requirement algebra: every
// requirement list is reduced on the host to one entry per (normalised) key
// — complement flag, Gt/Lt bounds and a sorted list of dense value ids — and
// the kernel evaluates Requirements.Compatible for each (claim, instance
// type) pair by merging the two key-sorted lists (one lane per pair).
//
// HBM layout (gs_create_filter: one arena per call):
//   reqs[]  FReq (32 B) — all requirement lists, key-sorted within a list
//   vals[]  u32 dense value ids, sorted within a requirement
//   vint[]  i64 parsed value (strconv.Atoi) per dense value, vok[] u8 parse ok
//   its[]   FIt: requirement list, offering range, Allocatable() < 0 flag
//   offs[]  FOff: requirement list, Available, Requirements.Get(ct).Has(spot)
//   alloc[] i64 [N][R]: Allocatable() over the resources the claims request
//   qs[]    FQuery: requirement list + request range into qty[]
//   out     u64 bitsets [Q][W] x3 (Create filter, requirements-only, spot)
//
// The prepared form splits the arena in two.  The catalog part (reqs, vals,
// vint, vok, its, offs, alloc over every resource a capacity list names)
// stays on the device from gs_create_filter_prepare on; a run uploads only
// the claims' part (their reqs, vals, the vint / vok of values the catalog
// does not know, qs, qty) and reads back one 16-B record per claim, plus the
// Create and requirements bitsets under GS_CF_BITSETS.  Keys and values the
// catalog knows keep the ids the prepare gave them; the others get ids above
// the catalog's for the one call.
#include "ctx.hpp"

#include <map>
#include <set>

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

struct DevFilter {
  const FReq* reqs;
  const uint32_t* vals;
  const int64_t* vint;
  const uint8_t* vok;
  const FIt* its;
  const FOff* offs;
  const int64_t* alloc;
  const FQuery* qs;
  const FQty* qty;
  uint32_t N, Q, R, W;
  uint64_t* out_create;
  uint64_t* out_reqs;
  uint64_t* out_spot;
  __device__ bool vok_at(uint32_t v) const { return vok[v]; }
  __device__ int64_t vint_at(uint32_t v) const { return vint[v]; }
};

// claim_select_kernel's claim staging budget (LDS per workgroup): a claim
// whose reduced list has at most kSelLdsReqs keys and kSelLdsVals values in
// all is copied to LDS once (1 KiB + 4 KiB); a longer one is read from HBM
constexpr uint32_t kSelLdsReqs = 32, kSelLdsVals = 1024;
__host__ __device__ inline bool sel_fits_lds(uint32_t n_reqs, uint32_t n_vals) {
  return n_reqs <= kSelLdsReqs && n_vals <= kSelLdsVals;
}

// one claim's outcome (claim_select_kernel): 16 B
struct FRec {
  uint32_t n_compatible;
  int32_t selected;
  uint32_t capacity_type, zero;
};
static_assert(sizeof(FRec) == 16, "filter record");

// The prepared form's two halves.  Dense value ids below V are the resident
// catalog's (c_vint / c_vok), the others the call's (q_vint / q_vok at id - V);
// a requirement's vb indexes the vals array of the half it came from.
struct DevSelect {
  const FReq* c_reqs;
  const uint32_t* c_vals;
  const int64_t* c_vint;
  const uint8_t* c_vok;
  const FIt* its;
  const FOff* offs;
  const int64_t* alloc;
  uint32_t N, R, W, V;
  const FReq* q_reqs;
  const uint32_t* q_vals;
  const int64_t* q_vint;
  const uint8_t* q_vok;
  const FQuery* qs;
  const FQty* qty;
  FRec* out_rec;
  uint64_t* out_create;  // nullptr without GS_CF_BITSETS
  uint64_t* out_reqs;
  __device__ bool vok_at(uint32_t v) const { return v < V ? c_vok[v] : q_vok[v - V]; }
  __device__ int64_t vint_at(uint32_t v) const { return v < V ? c_vint[v] : q_vint[v - V]; }
};

// ----------------------------------------------------------------- device
__device__ __forceinline__ bool exempt(const FReq& q) {
  // Operator() in {NotIn, DoesNotExist}
  return (q.flags & F_COMP) ? q.vn != 0 : q.vn == 0;
}

__device__ __forceinline__ bool contains(const uint32_t* v, uint32_t n, uint32_t x) {
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
__device__ bool len_zero(const D& d, const FReq& a, const uint32_t* av, const FReq& b, const uint32_t* bv) {
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
__device__ bool compatible(const D& d, const FReq* ex, uint32_t en, const uint32_t* exv, const FReq* in, uint32_t inn,
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

// one lane per (claim, instance type); blockIdx.y = claim, 256 types per block
__global__ __launch_bounds__(256) void claim_filter_kernel(DevFilter d) {
  const uint32_t q = blockIdx.y;
  const uint32_t it = blockIdx.x * 256 + threadIdx.x;
  bool ok_req = false, ok_create = false, ok_spot = false;
  if (it < d.N) {
    const FQuery Q = d.qs[q];
    const FIt I = d.its[it];
    const FReq* qr = d.reqs + Q.reqs.b;
    ok_req = compatible(d, qr, Q.reqs.n, d.vals, d.reqs + I.reqs.b, I.reqs.n, d.vals);
    bool fits = !I.alloc_neg;
    for (uint32_t k = 0; fits && k < Q.qn; k++) {
      const FQty x = d.qty[Q.qb + k];
      fits = x.v <= d.alloc[(size_t)it * d.R + x.r];
    }
    bool any = false;
    for (uint32_t o = 0; ok_req && fits && o < I.on; o++) {
      const FOff f = d.offs[I.ob + o];
      if (!f.available || !compatible(d, qr, Q.reqs.n, d.vals, d.reqs + f.reqs.b, f.reqs.n, d.vals)) continue;
      any = true;
      if (f.spot) {
        ok_spot = true;
        break;
      }
    }
    ok_create = ok_req && fits && any;
    ok_spot = ok_spot && ok_create;
  }
  const uint64_t b_req = __ballot(ok_req), b_create = __ballot(ok_create), b_spot = __ballot(ok_spot);
  const uint32_t w = it >> 6;
  if ((threadIdx.x & 63) == 0 && w < d.W) {
    const size_t o = (size_t)q * d.W + w;
    d.out_reqs[o] = b_req;
    d.out_create[o] = b_create;
    d.out_spot[o] = b_spot;
  }
}

// The prepared form: one 256-thread workgroup per claim (blockIdx.x), looping
// over the instance types 256 at a time, one lane per pair.  The claim's list
// is staged in LDS when it fits sel_fits_lds (a per-workgroup choice, so the
// barrier after it is reached by every thread) and read from HBM otherwise.
// Per chunk the three wave ballots are the bitset words (stored only when the
// caller asked for bitsets); each wave keeps the Create ballot's population
// count, its lowest set index and whether a spot bit was set, the four waves
// meet in LDS, and thread 0 stores the claim's FRec.
__global__ __launch_bounds__(256) void claim_select_kernel(DevSelect d) {
  __shared__ FReq s_reqs[kSelLdsReqs];
  __shared__ uint32_t s_vals[kSelLdsVals];
  __shared__ uint32_t s_cnt[4], s_first[4], s_spot[4];
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const FQuery Q = d.qs[q];
  const bool staged = sel_fits_lds(Q.reqs.n, Q.vn);
  if (staged) {
    for (uint32_t i = t; i < Q.reqs.n; i += 256) {
      FReq r = d.q_reqs[Q.reqs.b + i];
      r.vb -= Q.vb;  // into s_vals
      s_reqs[i] = r;
    }
    for (uint32_t i = t; i < Q.vn; i += 256) s_vals[i] = d.q_vals[Q.vb + i];
  }
  __syncthreads();
  const FReq* qr = staged ? s_reqs : d.q_reqs + Q.reqs.b;
  const uint32_t* qv = staged ? s_vals : d.q_vals;
  uint32_t cnt = 0, first = ~0u, spot = 0;  // wave-uniform: they follow the ballots
  for (uint32_t base = 0; base < d.N; base += 256) {
    const uint32_t it = base + t;
    bool ok_req = false, ok_create = false, ok_spot = false;
    if (it < d.N) {
      const FIt I = d.its[it];
      ok_req = compatible(d, qr, Q.reqs.n, qv, d.c_reqs + I.reqs.b, I.reqs.n, d.c_vals);
      bool fits = !I.alloc_neg;
      for (uint32_t k = 0; fits && k < Q.qn; k++) {
        const FQty x = d.qty[Q.qb + k];
        // a resource no capacity list names: Allocatable() reads 0
        fits = x.v <= (x.r < d.R ? d.alloc[(size_t)it * d.R + x.r] : 0);
      }
      bool any = false;
      for (uint32_t o = 0; ok_req && fits && o < I.on; o++) {
        const FOff f = d.offs[I.ob + o];
        if (!f.available || !compatible(d, qr, Q.reqs.n, qv, d.c_reqs + f.reqs.b, f.reqs.n, d.c_vals)) continue;
        any = true;
        if (f.spot) {
          ok_spot = true;
          break;
        }
      }
      ok_create = ok_req && fits && any;
      ok_spot = ok_spot && ok_create;
    }
    const uint64_t b_req = __ballot(ok_req), b_create = __ballot(ok_create), b_spot = __ballot(ok_spot);
    const uint32_t w = it >> 6;
    if (d.out_create && (t & 63) == 0 && w < d.W) {
      const size_t o = (size_t)q * d.W + w;
      d.out_reqs[o] = b_req;
      d.out_create[o] = b_create;
    }
    if (b_create && first == ~0u) first = (it & ~63u) + (uint32_t)__builtin_ctzll(b_create);
    cnt += (uint32_t)__builtin_popcountll(b_create);
    spot |= b_spot != 0;
  }
  if ((t & 63) == 0) {
    s_cnt[t >> 6] = cnt;
    s_first[t >> 6] = first;
    s_spot[t >> 6] = spot;
  }
  __syncthreads();
  if (t == 0) {
    FRec r{};
    uint32_t f = ~0u, sp = 0;
    for (uint32_t w = 0; w < 4; w++) {
      r.n_compatible += s_cnt[w];
      f = s_first[w] < f ? s_first[w] : f;
      sp |= s_spot[w];
    }
    r.selected = (int32_t)f;  // ~0u: -1
    r.capacity_type = (Q.spot && sp) ? GS_CAPACITY_SPOT : GS_CAPACITY_ON_DEMAND;
    d.out_rec[q] = r;
  }
}

// ------------------------------------------------------------------- host
struct Fail {
  gs_status code;
  std::string msg;
};

// one requirement on one key during host reduction
struct HReq {
  uint32_t key;
  bool comp = true;
  std::vector<uint32_t> vals;  // sorted dense value ids
  bool hg = false, hl = false;
  int64_t gt = 0, lt = 0;
};

constexpr uint32_t kNone = ~0u;

// The reduction of one gs_problem's requirement lists.  With `base` set (a
// run against a prepared catalog) keys and values are looked up in the base's
// vocabularies first and only the unknown ones get ids here, above the base's
// (kb / vb); this object, and those ids with it, lives for one call.
struct Enc {
  const gs_problem* p;
  const Enc* base = nullptr;
  uint32_t kb = 0, vb = 0;  // base->key_name.size(), base->vint.size()
  std::map<std::string, uint32_t> key_id;
  std::vector<std::string> key_name;
  std::vector<uint8_t> key_wk;  // label_is_wellknown
  std::unordered_map<std::string, uint32_t> val_id;
  std::vector<int64_t> vint;
  std::vector<uint8_t> vok;
  std::vector<uint32_t> key_of, val_of;  // p's string id -> key / value id (kNone: not asked yet)
  std::vector<FReq> reqs;
  std::vector<uint32_t> vals;

  std::string S(uint32_t id) const {
    if (id >= p->n_strings) throw Fail{GS_E_INVALID, "string id out of range"};
    return p->strings[id] ? p->strings[id] : "";
  }
  void chk(gs_range r, uint32_t n, const char* what) const {
    if ((uint64_t)r.begin + r.count > n) throw Fail{GS_E_INVALID, std::string("range out of bounds: ") + what};
  }
  uint32_t value(const std::string& v) {
    if (base) {
      auto f = base->val_id.find(v);
      if (f != base->val_id.end()) return f->second;
    }
    auto f = val_id.find(v);
    if (f != val_id.end()) return f->second;
    const uint32_t id = vb + (uint32_t)vint.size();
    val_id.emplace(v, id);
    int64_t x = 0;
    vok.push_back(gsh::go_atoi64(v, &x) ? 1 : 0);
    vint.push_back(x);
    return id;
  }
  uint32_t value_of(uint32_t sid) {
    if (sid >= p->n_strings) throw Fail{GS_E_INVALID, "string id out of range"};
    if (val_of.empty()) val_of.assign(p->n_strings, kNone);
    if (val_of[sid] == kNone) val_of[sid] = value(S(sid));
    return val_of[sid];
  }
  uint32_t find_key(const std::string& k) const {
    if (base) {
      auto f = base->key_id.find(k);
      if (f != base->key_id.end()) return f->second;
    }
    auto f = key_id.find(k);
    return f == key_id.end() ? kNone : f->second;
  }
  // the id of a (not yet normalised) label key
  uint32_t key_of_string(uint32_t sid) {
    if (sid >= p->n_strings) throw Fail{GS_E_INVALID, "string id out of range"};
    if (key_of.empty()) key_of.assign(p->n_strings, kNone);
    if (key_of[sid] != kNone) return key_of[sid];
    const std::string k = gsh::label_normalize(S(sid));
    uint32_t id = find_key(k);
    if (id == kNone) {
      id = kb + (uint32_t)key_name.size();
      key_id.emplace(k, id);
      key_name.push_back(k);
      key_wk.push_back(gsh::label_is_wellknown(k) ? 1 : 0);
    }
    return key_of[sid] = id;
  }
  bool wellknown(uint32_t key) const { return key < kb ? base->key_wk[key] : key_wk[key - kb]; }
  bool vok_at(uint32_t v) const { return v < vb ? base->vok[v] : vok[v - vb]; }
  int64_t vint_at(uint32_t v) const { return v < vb ? base->vint[v] : vint[v - vb]; }
  bool within(uint32_t v, bool hg, int64_t gt, bool hl, int64_t lt) const {
    if (!hg && !hl) return true;
    if (!vok_at(v)) return false;
    return !(hg && gt >= vint_at(v)) && !(hl && lt <= vint_at(v));
  }
  // <U> NewRequirement (keys normalised, In/NotIn values, Gt/Lt bounds)
  HReq make(const gs_requirement& q) {
    if (q.op > GS_OP_LTE) throw Fail{GS_E_INVALID, "unknown requirement operator"};
    // minValues: Compatible ignores it (reference cloudprovider.go:321-325)
    chk(q.values, p->n_value_ids, "values");
    HReq r;
    r.key = key_of_string(q.key);
    r.comp = !(q.op == GS_OP_IN || q.op == GS_OP_DOES_NOT_EXIST);
    if (q.op == GS_OP_IN || q.op == GS_OP_NOTIN) {
      for (uint32_t i = 0; i < q.values.count; i++) r.vals.push_back(value_of(p->value_ids[q.values.begin + i]));
      std::sort(r.vals.begin(), r.vals.end());
      r.vals.erase(std::unique(r.vals.begin(), r.vals.end()), r.vals.end());
    }
    if (q.op >= GS_OP_GT) {
      int64_t x = 0;
      if (q.values.count < 1 || !gsh::go_atoi64(S(p->value_ids[q.values.begin]), &x))
        throw Fail{GS_E_INVALID, "Gt/Lt/Gte/Lte value is not an integer"};
      if ((q.op == GS_OP_GTE && x == INT64_MIN) || (q.op == GS_OP_LTE && x == INT64_MAX))
        throw Fail{GS_E_INVALID, "Gte/Lte bound out of range"};
      // over integer label values Gte x is Gt x-1 and Lte x is Lt x+1
      const bool lower = q.op == GS_OP_GT || q.op == GS_OP_GTE;
      const int64_t b = q.op == GS_OP_GTE ? x - 1 : q.op == GS_OP_LTE ? x + 1 : x;
      (lower ? r.hg : r.hl) = true;
      (lower ? r.gt : r.lt) = b;
    }
    return r;
  }
  // <U> Requirement.Intersection (Requirements.Add on a repeated key)
  HReq intersect(const HReq& a, const HReq& b) const {
    HReq r;
    r.key = a.key;
    r.hg = a.hg || b.hg;
    r.gt = a.hg && b.hg ? std::max(a.gt, b.gt) : (a.hg ? a.gt : b.gt);
    r.hl = a.hl || b.hl;
    r.lt = a.hl && b.hl ? std::min(a.lt, b.lt) : (a.hl ? a.lt : b.lt);
    if (r.hg && r.hl && r.gt >= r.lt) {  // DoesNotExist
      r.comp = false;
      r.hg = r.hl = false;
      return r;
    }
    r.comp = a.comp && b.comp;
    std::vector<uint32_t> v;
    if (a.comp && b.comp)
      std::set_union(a.vals.begin(), a.vals.end(), b.vals.begin(), b.vals.end(), std::back_inserter(v));
    else if (a.comp)
      std::set_difference(b.vals.begin(), b.vals.end(), a.vals.begin(), a.vals.end(), std::back_inserter(v));
    else if (b.comp)
      std::set_difference(a.vals.begin(), a.vals.end(), b.vals.begin(), b.vals.end(), std::back_inserter(v));
    else
      std::set_intersection(a.vals.begin(), a.vals.end(), b.vals.begin(), b.vals.end(), std::back_inserter(v));
    for (uint32_t x : v)
      if (within(x, r.hg, r.gt, r.hl, r.lt)) r.vals.push_back(x);
    if (!r.comp) r.hg = r.hl = false;
    return r;
  }
  // NewNodeSelectorRequirementsWithMinValues: one entry per key
  std::map<uint32_t, HReq> reduce(gs_range rg) {
    chk(rg, p->n_reqs, "reqs");
    std::map<uint32_t, HReq> m;
    for (uint32_t i = 0; i < rg.count; i++) {
      HReq r = make(p->reqs[rg.begin + i]);
      auto f = m.find(r.key);
      if (f == m.end()) m.emplace(r.key, std::move(r));
      else f->second = intersect(r, f->second);
    }
    return m;
  }
  FList emit(const std::map<uint32_t, HReq>& m) {
    FList l{(uint32_t)reqs.size(), (uint32_t)m.size()};
    for (auto& kv : m) {
      const HReq& r = kv.second;
      FReq f{};
      f.key = r.key;
      f.flags = (r.comp ? F_COMP : 0) | (r.hg ? F_GT : 0) | (r.hl ? F_LT : 0) | (wellknown(r.key) ? F_WK : 0);
      f.vb = (uint32_t)vals.size();
      f.vn = (uint32_t)r.vals.size();
      f.gt = r.gt;
      f.lt = r.lt;
      vals.insert(vals.end(), r.vals.begin(), r.vals.end());
      reqs.push_back(f);
    }
    return l;
  }
  // Requirements.Get(capacity-type).Has("spot") (absent key: Exists)
  bool has_spot(const std::map<uint32_t, HReq>& m) {
    const uint32_t k = find_key("karpenter.sh/capacity-type");
    if (k == kNone) return true;
    auto f = m.find(k);
    if (f == m.end()) return true;
    const HReq& r = f->second;
    const uint32_t v = value("spot");
    const bool in = std::binary_search(r.vals.begin(), r.vals.end(), v);
    return (r.comp ? !in : in) && within(v, r.hg, r.gt, r.hl, r.lt);
  }
};

// the claims' half: reduced lists and summed requests.  res(name) gives a
// requested resource's column of alloc[] (or any id at or past R for a name
// no column stands for).
template <class Res>
void encode_claims(Enc& e, const gs_claim_query* qs, uint32_t nq, Res res, std::vector<FQuery>& fq,
                   std::vector<FQty>& qty) {
  const gs_problem* p = e.p;
  for (uint32_t q = 0; q < nq; q++) {
    auto m = e.reduce(qs[q].requirements);
    FQuery x{};
    x.vb = (uint32_t)e.vals.size();
    x.reqs = e.emit(m);
    x.vn = (uint32_t)e.vals.size() - x.vb;
    x.spot = e.has_spot(m) ? 1 : 0;
    e.chk(qs[q].requests, p->n_quantities, "requests");
    std::map<uint32_t, int64_t> sum;  // resource lists are maps: repeated names add
    for (uint32_t k = 0; k < qs[q].requests.count; k++) {
      const gs_quantity& g = p->quantities[qs[q].requests.begin + k];
      sum[res(g.resource)] += g.milli;
    }
    x.qb = (uint32_t)qty.size();
    x.qn = (uint32_t)sum.size();
    for (auto& kv : sum) qty.push_back(FQty{kv.first, 0, kv.second});
    fq.push_back(x);
  }
}

// the catalog's half: every instance type's and offering's reduced list and
// Allocatable() over the resources of res_id ([N][R]).  slots (optional):
// per index of p->offerings, the positions in offs[] that stand for it (one
// per instance type whose range holds it).
void encode_catalog(Enc& e, const std::map<std::string, uint32_t>& res_id, uint32_t R, std::vector<FIt>& its,
                    std::vector<FOff>& offs, std::vector<int64_t>& alloc, std::vector<std::vector<uint32_t>>* slots) {
  const gs_problem* p = e.p;
  const uint32_t N = p->n_instance_types;
  alloc.assign((size_t)N * R, 0);
  e.chk(gs_range{0, N}, N, "instance_types");
  for (uint32_t i = 0; i < N; i++) {
    const gs_instance_type& g = p->instance_types[i];
    FIt x{};
    x.reqs = e.emit(e.reduce(g.requirements));
    // Allocatable() = capacity - overhead over the capacity's resources
    e.chk(g.capacity, p->n_quantities, "capacity");
    e.chk(g.overhead, p->n_quantities, "overhead");
    std::map<std::string, int64_t> cap, ovh;
    for (uint32_t k = 0; k < g.capacity.count; k++)
      cap[e.S(p->quantities[g.capacity.begin + k].resource)] += p->quantities[g.capacity.begin + k].milli;
    for (uint32_t k = 0; k < g.overhead.count; k++)
      ovh[e.S(p->quantities[g.overhead.begin + k].resource)] += p->quantities[g.overhead.begin + k].milli;
    for (auto& kv : cap) {
      auto o = ovh.find(kv.first);
      const int64_t a = kv.second - (o == ovh.end() ? 0 : o->second);
      if (a < 0) x.alloc_neg = 1;
      auto r = res_id.find(kv.first);
      if (r != res_id.end()) alloc[(size_t)i * R + r->second] = a;
    }
    e.chk(g.offerings, p->n_offerings, "offerings");
    x.ob = (uint32_t)offs.size();
    x.on = g.offerings.count;
    for (uint32_t k = 0; k < g.offerings.count; k++) {
      const gs_offering& o = p->offerings[g.offerings.begin + k];
      auto m = e.reduce(o.requirements);
      FOff f{};
      f.reqs = e.emit(m);
      f.available = o.available ? 1 : 0;
      f.spot = e.has_spot(m) ? 1 : 0;
      if (slots) (*slots)[g.offerings.begin + k].push_back((uint32_t)offs.size());
      offs.push_back(f);
    }
    its.push_back(x);
  }
}

// an image of 256-B aligned sub-buffers, uploaded with one copy
struct Image {
  size_t off = 0;
  size_t place(size_t bytes) {
    const size_t o = off;
    off += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    return o;
  }
};
template <class T>
void put(char* h, size_t o, const std::vector<T>& v) {
  if (!v.empty()) std::memcpy(h + o, v.data(), v.size() * sizeof(T));
}

// gs_create_filter_prepare's catalog, resident on the device, and the
// buffers and results of the runs against it
struct Resident {
  bool ready = false;
  Enc voc;                                // the catalog's key and value vocabularies (no lists)
  std::map<std::string, uint32_t> res_id;  // alloc[] columns: every resource a capacity list names
  uint32_t N = 0, R = 1, W = 0;
  std::vector<FOff> offs;                      // host mirror of the device array
  std::vector<std::vector<uint32_t>> slots;    // catalog offering index -> positions in offs
  void* cat_dev = nullptr;                     // the catalog image
  size_t o_reqs = 0, o_vals = 0, o_vint = 0, o_vok = 0, o_its = 0, o_offs = 0, o_alloc = 0;
  // a run's claim image and outputs: grow-once device arena, pinned host sides
  void* run_dev = nullptr;
  size_t run_bytes = 0;
  void* h_in = nullptr;
  size_t h_in_bytes = 0;
  void* h_out = nullptr;
  size_t h_out_bytes = 0;
  std::vector<uint32_t> res_n, res_ct;
  std::vector<int32_t> res_sel;
  gs_create_filter_stats stats{};
};

}  // namespace gsf

using namespace gsc;
using namespace gsf;

static void grow_pinned(void*& p, size_t& cap, size_t want) {
  if (want <= cap) return;
  if (p) HIPCHK(hipHostFree(p));
  p = nullptr;
  cap = 0;
  HIPCHK(hipHostMalloc(&p, want + want / 4, hipHostMallocDefault));
  cap = want + want / 4;
}

void gsc::create_filter_destroy(gs_ctx* c) {
  if (c->cf_dev) (void)hipFree(c->cf_dev);
  c->cf_dev = nullptr;
  Resident* r = c->cf_res;
  if (!r) return;
  if (r->cat_dev) (void)hipFree(r->cat_dev);
  if (r->run_dev) (void)hipFree(r->run_dev);
  if (r->h_in) (void)hipHostFree(r->h_in);
  if (r->h_out) (void)hipHostFree(r->h_out);
  delete r;
  c->cf_res = nullptr;
}

static bool null_with_count(const gs_problem* p, bool catalog) {
  return (catalog && ((p->n_instance_types && !p->instance_types) || (p->n_offerings && !p->offerings))) ||
         (p->n_quantities && !p->quantities) || (p->n_reqs && !p->reqs) || (p->n_value_ids && !p->value_ids) ||
         (p->n_strings && !p->strings);
}

extern "C" gs_status gs_create_filter(gs_ctx* c, const gs_problem* p, const gs_claim_query* qs, uint32_t nq,
                                      gs_claim_filter_result* out) {
  if (!c || !p || !out || (nq && !qs)) return GS_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  // reject before any allocation: the grid's y dimension, and every array the
  // host pass reads that is null while its count is not
  if (nq > 65535u) return fail(c, GS_E_INVALID, "more than 65535 claims in one gs_create_filter call");
  if (null_with_count(p, true)) return fail(c, GS_E_INVALID, "null array with a non-zero count");
  Enc e;
  e.p = p;
  std::vector<FIt> its;
  std::vector<FOff> offs;
  std::vector<FQuery> fq;
  std::vector<FQty> qty;
  std::vector<int64_t> alloc;
  uint32_t R = 0;
  const uint32_t N = p->n_instance_types;
  try {
    // claims first: their requested resources form the Fits vocabulary
    std::map<std::string, uint32_t> res_id;
    encode_claims(
        e, qs, nq, [&](uint32_t sid) { return res_id.emplace(e.S(sid), (uint32_t)res_id.size()).first->second; }, fq, qty);
    R = std::max<uint32_t>(1, (uint32_t)res_id.size());
    encode_catalog(e, res_id, R, its, offs, alloc, nullptr);
  } catch (const Fail& f) {
    return fail(c, f.code, f.msg);
  }
  const uint32_t W = (N + 63) / 64;
  c->cf_create.assign((size_t)nq * W, 0);
  c->cf_reqs.assign((size_t)nq * W, 0);
  c->cf_spot.assign((size_t)nq * W, 0);
  if (nq && N) {
    try {
      HIPCHK(hipSetDevice(c->device));
      // one arena: inputs then the three output bitsets
      Image im;
      const size_t o_reqs = im.place(e.reqs.size() * sizeof(FReq)), o_vals = im.place(e.vals.size() * 4),
                   o_vint = im.place(e.vint.size() * 8), o_vok = im.place(e.vok.size()),
                   o_its = im.place(its.size() * sizeof(FIt)), o_offs = im.place(offs.size() * sizeof(FOff)),
                   o_alloc = im.place(alloc.size() * 8), o_qs = im.place(fq.size() * sizeof(FQuery)),
                   o_qty = im.place(qty.size() * sizeof(FQty)), o_out = im.place((size_t)3 * nq * W * 8);
      if (im.off > c->cf_bytes) {
        if (c->cf_dev) HIPCHK(hipFree(c->cf_dev));
        c->cf_dev = nullptr;
        c->cf_bytes = 0;
        HIPCHK(hipMalloc(&c->cf_dev, im.off));
        c->cf_bytes = im.off;
      }
      char* base = (char*)c->cf_dev;
      // staging: one host copy, one H2D transfer
      std::vector<char> h(o_out);
      put(h.data(), o_reqs, e.reqs);
      put(h.data(), o_vals, e.vals);
      put(h.data(), o_vint, e.vint);
      put(h.data(), o_vok, e.vok);
      put(h.data(), o_its, its);
      put(h.data(), o_offs, offs);
      put(h.data(), o_alloc, alloc);
      put(h.data(), o_qs, fq);
      put(h.data(), o_qty, qty);
      HIPCHK(hipMemcpyAsync(base, h.data(), o_out, hipMemcpyHostToDevice, c->stream));
      DevFilter d{};
      d.reqs = (const FReq*)(base + o_reqs);
      d.vals = (const uint32_t*)(base + o_vals);
      d.vint = (const int64_t*)(base + o_vint);
      d.vok = (const uint8_t*)(base + o_vok);
      d.its = (const FIt*)(base + o_its);
      d.offs = (const FOff*)(base + o_offs);
      d.alloc = (const int64_t*)(base + o_alloc);
      d.qs = (const FQuery*)(base + o_qs);
      d.qty = (const FQty*)(base + o_qty);
      d.N = N;
      d.Q = nq;
      d.R = R;
      d.W = W;
      d.out_create = (uint64_t*)(base + o_out);
      d.out_reqs = d.out_create + (size_t)nq * W;
      d.out_spot = d.out_reqs + (size_t)nq * W;
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      hipLaunchKernelGGL(claim_filter_kernel, dim3((N + 255) / 256, nq), dim3(256), 0, c->stream, d);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      const size_t ob = (size_t)nq * W * 8;
      HIPCHK(hipMemcpyAsync(c->cf_create.data(), d.out_create, ob, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(c->cf_reqs.data(), d.out_reqs, ob, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(c->cf_spot.data(), d.out_spot, ob, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
      c->t_filter = ms;
    } catch (const HipError& ex) {
      return fail(c, GS_E_HIP, ex.msg);
    }
  }
  c->cf_n.assign(nq, 0);
  c->cf_sel.assign(nq, -1);
  c->cf_ct.assign(nq, GS_CAPACITY_ON_DEMAND);
  for (uint32_t q = 0; q < nq; q++) {
    bool spot = false;
    for (uint32_t w = 0; w < W; w++) {
      const uint64_t x = c->cf_create[(size_t)q * W + w];
      if (x && c->cf_sel[q] < 0) c->cf_sel[q] = (int32_t)(64 * w + __builtin_ctzll(x));
      c->cf_n[q] += (uint32_t)__builtin_popcountll(x);
      spot |= c->cf_spot[(size_t)q * W + w] != 0;
    }
    if (fq[q].spot && spot) c->cf_ct[q] = GS_CAPACITY_SPOT;
  }
  out->n_queries = nq;
  out->words = W;
  out->compatible = c->cf_create.data();
  out->requirements = c->cf_reqs.data();
  out->n_compatible = c->cf_n.data();
  out->selected = c->cf_sel.data();
  out->capacity_type = c->cf_ct.data();
  return GS_OK;
}

// ------------------------------------------------------- the prepared form
extern "C" uint32_t gs_create_filter_stats_size(void) { return (uint32_t)sizeof(gs_create_filter_stats); }

extern "C" gs_status gs_create_filter_last_run(const gs_ctx* c, gs_create_filter_stats* out) {
  if (!c || !out) return GS_E_INVALID;
  *out = c->cf_res ? c->cf_res->stats : gs_create_filter_stats{};
  return GS_OK;
}

extern "C" gs_status gs_create_filter_prepare(gs_ctx* c, const gs_problem* p) {
  if (!c || !p) return GS_E_INVALID;
  if (null_with_count(p, true)) return fail(c, GS_E_INVALID, "null array with a non-zero count");
  // the host encoding first: a failure leaves the resident catalog as it was
  const auto t0 = Clock::now();
  Enc e;
  e.p = p;
  std::map<std::string, uint32_t> res_id;
  std::vector<FIt> its;
  std::vector<FOff> offs;
  std::vector<int64_t> alloc;
  std::vector<std::vector<uint32_t>> slots(p->n_offerings);
  const uint32_t N = p->n_instance_types;
  uint32_t R = 1;
  try {
    e.chk(gs_range{0, N}, N, "instance_types");
    for (uint32_t i = 0; i < N; i++) {
      const gs_range cap = p->instance_types[i].capacity;
      e.chk(cap, p->n_quantities, "capacity");
      for (uint32_t k = 0; k < cap.count; k++)
        res_id.emplace(e.S(p->quantities[cap.begin + k].resource), (uint32_t)res_id.size());
    }
    R = std::max<uint32_t>(1, (uint32_t)res_id.size());
    encode_catalog(e, res_id, R, its, offs, alloc, &slots);
  } catch (const Fail& f) {
    return fail(c, f.code, f.msg);
  }
  Image im;
  const size_t o_reqs = im.place(e.reqs.size() * sizeof(FReq)), o_vals = im.place(e.vals.size() * 4),
               o_vint = im.place(e.vint.size() * 8), o_vok = im.place(e.vok.size()),
               o_its = im.place(its.size() * sizeof(FIt)), o_offs = im.place(offs.size() * sizeof(FOff)),
               o_alloc = im.place(alloc.size() * 8);
  std::vector<char> h(im.off);
  put(h.data(), o_reqs, e.reqs);
  put(h.data(), o_vals, e.vals);
  put(h.data(), o_vint, e.vint);
  put(h.data(), o_vok, e.vok);
  put(h.data(), o_its, its);
  put(h.data(), o_offs, offs);
  put(h.data(), o_alloc, alloc);
  const double encode_ms = ms_since(t0);
  const auto t1 = Clock::now();
  void* dev = nullptr;
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(&dev, im.off));
    HIPCHK(hipMemcpyAsync(dev, h.data(), im.off, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // also: no run of the old catalog is in flight
  } catch (const HipError& ex) {
    if (dev) (void)hipFree(dev);
    return fail(c, GS_E_HIP, ex.msg);
  }
  if (!c->cf_res) c->cf_res = new Resident;
  Resident& r = *c->cf_res;
  if (r.cat_dev) (void)hipFree(r.cat_dev);
  r.cat_dev = dev;
  // keep the vocabularies; the lists live on the device now
  e.p = nullptr;
  e.reqs = {};
  e.vals = {};
  e.key_of = {};
  e.val_of = {};
  r.voc = std::move(e);
  r.res_id = std::move(res_id);
  r.N = N;
  r.R = R;
  r.W = (N + 63) / 64;
  r.offs = std::move(offs);
  r.slots = std::move(slots);
  r.o_reqs = o_reqs;
  r.o_vals = o_vals;
  r.o_vint = o_vint;
  r.o_vok = o_vok;
  r.o_its = o_its;
  r.o_offs = o_offs;
  r.o_alloc = o_alloc;
  r.ready = true;
  r.stats = gs_create_filter_stats{};
  r.stats.encode_ms = encode_ms;
  r.stats.upload_ms = ms_since(t1);
  r.stats.h2d_bytes = im.off;
  r.stats.n_instance_types = N;
  return GS_OK;
}

extern "C" gs_status gs_create_filter_set_available(gs_ctx* c, const uint32_t* offering, const uint8_t* available,
                                                    uint32_t n) {
  if (!c || (n && (!offering || !available))) return GS_E_INVALID;
  Resident* r = c->cf_res;
  if (!r || !r->ready)
    return fail(c, GS_E_INVALID, "gs_create_filter_set_available before gs_create_filter_prepare");
  for (uint32_t i = 0; i < n; i++)
    if (offering[i] >= r->slots.size()) return fail(c, GS_E_INVALID, "offering index out of range");
  if (!n) return GS_OK;
  for (uint32_t i = 0; i < n; i++)  // in order: a repeated index takes its last value
    for (uint32_t s : r->slots[offering[i]]) r->offs[s].available = available[i] ? 1 : 0;
  if (r->offs.empty()) return GS_OK;
  try {
    HIPCHK(hipSetDevice(c->device));
    // the whole FOff array (16 B per offering) from the patched mirror: one
    // transfer whatever n is, on the stream the next run is launched on
    HIPCHK(hipMemcpyAsync((char*)r->cat_dev + r->o_offs, r->offs.data(), r->offs.size() * sizeof(FOff),
                          hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // the mirror may change again after this call
  } catch (const HipError& ex) {
    return fail(c, GS_E_HIP, ex.msg);
  }
  return GS_OK;
}

extern "C" gs_status gs_create_filter_run(gs_ctx* c, const gs_problem* p, const gs_claim_query* qs, uint32_t nq,
                                          uint32_t flags, gs_claim_filter_result* out) {
  if (!c || !p || !out || (nq && !qs)) return GS_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  Resident* rp = c->cf_res;
  if (!rp || !rp->ready) return fail(c, GS_E_INVALID, "gs_create_filter_run before gs_create_filter_prepare");
  Resident& r = *rp;
  if (flags & ~GS_CF_BITSETS) return fail(c, GS_E_INVALID, "unknown gs_create_filter_run flag");
  if (nq > 65535u) return fail(c, GS_E_INVALID, "more than 65535 claims in one gs_create_filter_run call");
  if (null_with_count(p, false)) return fail(c, GS_E_INVALID, "null array with a non-zero count");
  const auto t0 = Clock::now();
  // ids for this call only: e goes when the call returns
  Enc e;
  e.p = p;
  e.base = &r.voc;
  e.kb = (uint32_t)r.voc.key_name.size();
  e.vb = (uint32_t)r.voc.vint.size();
  std::vector<FQuery> fq;
  std::vector<FQty> qty;
  try {
    std::vector<uint32_t> res_of(p->n_strings, kNone);  // the pool's string id -> alloc column
    std::map<std::string, uint32_t> unknown;             // names no capacity list has: columns past R
    encode_claims(
        e, qs, nq,
        [&](uint32_t sid) {
          if (sid >= p->n_strings) throw Fail{GS_E_INVALID, "string id out of range"};
          if (res_of[sid] == kNone) {
            const std::string name = e.S(sid);
            auto f = r.res_id.find(name);
            res_of[sid] = f != r.res_id.end() ? f->second
                                              : r.R + unknown.emplace(name, (uint32_t)unknown.size()).first->second;
          }
          return res_of[sid];
        },
        fq, qty);
  } catch (const Fail& f) {
    return fail(c, f.code, f.msg);
  }
  uint32_t n_staged = 0;
  for (const FQuery& x : fq) n_staged += sel_fits_lds(x.reqs.n, x.vn) ? 1 : 0;
  const bool bits = flags & GS_CF_BITSETS;
  const uint32_t W = r.W;
  gs_create_filter_stats st{};
  st.n_queries = nq;
  st.n_instance_types = r.N;
  st.n_staged_lds = n_staged;
  r.res_n.assign(nq, 0);
  r.res_sel.assign(nq, -1);
  r.res_ct.assign(nq, GS_CAPACITY_ON_DEMAND);
  const uint64_t* h_create = nullptr;
  const uint64_t* h_reqs = nullptr;
  if (nq) {
    try {
      HIPCHK(hipSetDevice(c->device));
      // the claims' image, then the outputs: records, and the two bitsets when asked for
      Image im;
      const size_t o_reqs = im.place(e.reqs.size() * sizeof(FReq)), o_vals = im.place(e.vals.size() * 4),
                   o_vint = im.place(e.vint.size() * 8), o_vok = im.place(e.vok.size()),
                   o_qs = im.place(fq.size() * sizeof(FQuery)), o_qty = im.place(qty.size() * sizeof(FQty));
      const size_t in_bytes = im.off;
      const size_t bs_bytes = bits ? (size_t)nq * W * 8 : 0;
      const size_t out_bytes = (size_t)nq * sizeof(FRec) + 2 * bs_bytes;
      if (in_bytes + out_bytes > r.run_bytes) {
        if (r.run_dev) HIPCHK(hipFree(r.run_dev));
        r.run_dev = nullptr;
        r.run_bytes = 0;
        const size_t want = in_bytes + out_bytes + (in_bytes + out_bytes) / 4;
        HIPCHK(hipMalloc(&r.run_dev, want));
        r.run_bytes = want;
      }
      grow_pinned(r.h_in, r.h_in_bytes, in_bytes);
      grow_pinned(r.h_out, r.h_out_bytes, out_bytes);
      char* h = (char*)r.h_in;
      put(h, o_reqs, e.reqs);
      put(h, o_vals, e.vals);
      put(h, o_vint, e.vint);
      put(h, o_vok, e.vok);
      put(h, o_qs, fq);
      put(h, o_qty, qty);
      st.encode_ms = ms_since(t0);
      const auto t1 = Clock::now();
      char* base = (char*)r.run_dev;
      const char* cat = (const char*)r.cat_dev;
      HIPCHK(hipMemcpyAsync(base, h, in_bytes, hipMemcpyHostToDevice, c->stream));
      st.h2d_bytes = in_bytes;
      DevSelect d{};
      d.c_reqs = (const FReq*)(cat + r.o_reqs);
      d.c_vals = (const uint32_t*)(cat + r.o_vals);
      d.c_vint = (const int64_t*)(cat + r.o_vint);
      d.c_vok = (const uint8_t*)(cat + r.o_vok);
      d.its = (const FIt*)(cat + r.o_its);
      d.offs = (const FOff*)(cat + r.o_offs);
      d.alloc = (const int64_t*)(cat + r.o_alloc);
      d.N = r.N;
      d.R = r.R;
      d.W = W;
      d.V = e.vb;
      d.q_reqs = (const FReq*)(base + o_reqs);
      d.q_vals = (const uint32_t*)(base + o_vals);
      d.q_vint = (const int64_t*)(base + o_vint);
      d.q_vok = (const uint8_t*)(base + o_vok);
      d.qs = (const FQuery*)(base + o_qs);
      d.qty = (const FQty*)(base + o_qty);
      d.out_rec = (FRec*)(base + in_bytes);
      if (bits) {
        d.out_create = (uint64_t*)(base + in_bytes + (size_t)nq * sizeof(FRec));
        d.out_reqs = d.out_create + (size_t)nq * W;
      }
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      hipLaunchKernelGGL(claim_select_kernel, dim3(nq), dim3(256), 0, c->stream, d);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      st.n_launches = 1;
      st.upload_ms = ms_since(t1);
      const auto t2 = Clock::now();
      HIPCHK(hipMemcpyAsync(r.h_out, base + in_bytes, out_bytes, hipMemcpyDeviceToHost, c->stream));
      st.d2h_bytes = out_bytes;
      HIPCHK(hipStreamSynchronize(c->stream));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
      st.kernel_ms = ms;
      const FRec* rec = (const FRec*)r.h_out;
      for (uint32_t q = 0; q < nq; q++) {
        r.res_n[q] = rec[q].n_compatible;
        r.res_sel[q] = rec[q].selected;
        r.res_ct[q] = rec[q].capacity_type;
      }
      if (bits) {
        h_create = (const uint64_t*)((const char*)r.h_out + (size_t)nq * sizeof(FRec));
        h_reqs = h_create + (size_t)nq * W;
      }
      st.fetch_ms = ms_since(t2);
    } catch (const HipError& ex) {
      return fail(c, GS_E_HIP, ex.msg);
    }
  } else {
    st.encode_ms = ms_since(t0);
  }
  r.stats = st;
  out->n_queries = nq;
  out->words = W;
  out->compatible = h_create;
  out->requirements = h_reqs;
  out->n_compatible = r.res_n.data();
  out->selected = r.res_sel.data();
  out->capacity_type = r.res_ct.data();
  return GS_OK;
}
