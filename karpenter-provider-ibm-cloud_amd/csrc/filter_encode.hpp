// filter_encode.hpp — the Create re-filter's host side that needs nothing
// from HIP: the reduction of a gs_problem's requirement lists to the records
// of filter_rules.hpp (filter_encode.cpp), and the two images the entry
// points of filter.hip upload.  Built by hipcc into the library and by plain
// g++ (with sanitizers) into tools/encode_harness.cpp.
//
// Unlike the Solve encoder (encode.cpp), which folds requirements into
// per-key vocabulary bitsets under the restrictions the FFD kernels need,
// this path keeps the general <U> scheduling.Requirement algebra.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "encode.hpp"
#include "filter_rules.hpp"

namespace gsf {

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
  uint32_t value(const std::string& v);
  uint32_t value_of(uint32_t sid);
  uint32_t find_key(const std::string& k) const;
  // the id of a (not yet normalised) label key
  uint32_t key_of_string(uint32_t sid);
  bool wellknown(uint32_t key) const { return key < kb ? base->key_wk[key] : key_wk[key - kb]; }
  bool vok_at(uint32_t v) const { return v < vb ? base->vok[v] : vok[v - vb]; }
  int64_t vint_at(uint32_t v) const { return v < vb ? base->vint[v] : vint[v - vb]; }
  bool within(uint32_t v, bool hg, int64_t gt, bool hl, int64_t lt) const {
    if (!hg && !hl) return true;
    if (!vok_at(v)) return false;
    return !(hg && gt >= vint_at(v)) && !(hl && lt <= vint_at(v));
  }
  // <U> NewRequirement (keys normalised, In/NotIn values, Gt/Lt bounds)
  HReq make(const gs_requirement& q);
  // <U> Requirement.Intersection (Requirements.Add on a repeated key)
  HReq intersect(const HReq& a, const HReq& b) const;
  // NewNodeSelectorRequirementsWithMinValues: one entry per key
  std::map<uint32_t, HReq> reduce(gs_range rg);
  FList emit(const std::map<uint32_t, HReq>& m);
  // Requirements.Get(capacity-type).Has("spot") (absent key: Exists)
  bool has_spot(const std::map<uint32_t, HReq>& m);
};

// a null array of p with a non-zero count, among those the reduction reads
// (catalog: the instance types and offerings too)
bool null_with_count(const gs_problem* p, bool catalog);

// Where a claim's requested resource lives in alloc[] ([N][R]).
struct Columns {
  // call_column, capacity_columns: resource name -> column; resident_column:
  // the names no column stands for
  std::map<std::string, uint32_t> id;
  uint32_t R = 1;                     // capacity_columns: the columns of alloc[]
  const Columns* catalog = nullptr;   // resident_column: the prepared catalog's columns
  std::vector<uint32_t> of;           // resident_column: the pool's string id -> column
};
// gs_create_filter: the claims come first and their requested resources form
// the Fits vocabulary, a column per name in order of first request
uint32_t call_column(const Enc& e, Columns& c, uint32_t sid);
// gs_create_filter_run: the columns are c.catalog's; a name no capacity list
// has gets an id at or past its R
uint32_t resident_column(const Enc& e, Columns& c, uint32_t sid);
// gs_create_filter_prepare: a column for every resource a capacity list names
void capacity_columns(const Enc& e, Columns& c);

// the claims' half: reduced lists and summed requests; col gives a requested
// resource's column of alloc[]
void encode_claims(Enc& e, const gs_claim_query* qs, uint32_t nq, uint32_t (*col)(const Enc&, Columns&, uint32_t),
                   Columns& c, std::vector<FQuery>& fq, std::vector<FQty>& qty);

// the catalog's half: every instance type's and offering's reduced list and
// Allocatable() over the resources of res_id ([N][R]).  slots (optional):
// per index of p->offerings, the positions in offs[] that stand for it (one
// per instance type whose range holds it).
void encode_catalog(Enc& e, const std::map<std::string, uint32_t>& res_id, uint32_t R, std::vector<FIt>& its,
                    std::vector<FOff>& offs, std::vector<int64_t>& alloc, std::vector<std::vector<uint32_t>>* slots);

// an image of 256-B aligned sub-buffers, uploaded with one copy
struct Image {
  size_t off = 0;
  size_t place(size_t bytes) {
    const size_t o = off;
    off += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    return o;
  }
  template <class T>
  size_t place(const std::vector<T>& v) {
    return place(v.size() * sizeof(T));
  }
};
template <class T>
void put(char* h, size_t o, const std::vector<T>& v) {
  if (!v.empty()) std::memcpy(h + o, v.data(), v.size() * sizeof(T));
}
template <class T>
const T* at(const char* base, size_t o) {
  return (const T*)(base + o);
}

// The catalog's part of an arena: reqs, vals, vint, vok, its, offs, alloc.
// The constructor places them in `im` (offsets from the image's start),
// fill() copies them to a host buffer, bind() points a DevFilter / DevSelect
// (or the harness's host view) at them under a base address.
struct CatalogImage {
  size_t reqs = 0, vals = 0, vint = 0, vok = 0, its = 0, offs = 0, alloc = 0;
  CatalogImage() = default;
  CatalogImage(Image& im, const Enc& e, const std::vector<FIt>& i, const std::vector<FOff>& o,
               const std::vector<int64_t>& a)
      : reqs(im.place(e.reqs)), vals(im.place(e.vals)), vint(im.place(e.vint)), vok(im.place(e.vok)),
        its(im.place(i)), offs(im.place(o)), alloc(im.place(a)) {}
  void fill(char* h, const Enc& e, const std::vector<FIt>& i, const std::vector<FOff>& o,
            const std::vector<int64_t>& a) const {
    put(h, reqs, e.reqs);
    put(h, vals, e.vals);
    put(h, vint, e.vint);
    put(h, vok, e.vok);
    put(h, its, i);
    put(h, offs, o);
    put(h, alloc, a);
  }
  template <class D>
  void bind(const char* base, D& d) const {
    d.reqs = at<FReq>(base, reqs);
    d.vals = at<uint32_t>(base, vals);
    d.vint = at<int64_t>(base, vint);
    d.vok = at<uint8_t>(base, vok);
    d.its = at<FIt>(base, its);
    d.offs = at<FOff>(base, offs);
    d.alloc = at<int64_t>(base, alloc);
  }
};

// The claims' part: reqs, vals, vint, vok of the claims' own Enc, then qs and
// qty.  `lists` is null where one Enc holds both halves (gs_create_filter):
// the catalog image carries its lists and only qs and qty are placed here.
struct ClaimImage {
  size_t reqs = 0, vals = 0, vint = 0, vok = 0, qs = 0, qty = 0;
  ClaimImage(Image& im, const Enc* lists, const std::vector<FQuery>& q, const std::vector<FQty>& y) {
    if (lists) {
      reqs = im.place(lists->reqs);
      vals = im.place(lists->vals);
      vint = im.place(lists->vint);
      vok = im.place(lists->vok);
    }
    qs = im.place(q);
    qty = im.place(y);
  }
  void fill(char* h, const Enc* lists, const std::vector<FQuery>& q, const std::vector<FQty>& y) const {
    if (lists) {
      put(h, reqs, lists->reqs);
      put(h, vals, lists->vals);
      put(h, vint, lists->vint);
      put(h, vok, lists->vok);
    }
    put(h, qs, q);
    put(h, qty, y);
  }
  template <class D>
  void bind(const char* base, D& d) const {
    d.qs = at<FQuery>(base, qs);
    d.qty = at<FQty>(base, qty);
  }
  // ... and the claims' own lists, where the image holds them
  template <class D>
  void bind_lists(const char* base, D& d) const {
    d.q_reqs = at<FReq>(base, reqs);
    d.q_vals = at<uint32_t>(base, vals);
    d.q_vint = at<int64_t>(base, vint);
    d.q_vok = at<uint8_t>(base, vok);
  }
};

}  // namespace gsf
