// filter_encode.cpp — the Create re-filter's host reduction (filter_encode.hpp):
// every requirement list of the caller's arrays becomes one FReq per
// normalised key.  It parses caller-owned ranges and ids, so every index is
// checked before it is used; a bad one throws Fail{GS_E_INVALID}.
#include "filter_encode.hpp"

#include <iterator>

namespace gsf {

uint32_t Enc::value(const std::string& v) {
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

uint32_t Enc::value_of(uint32_t sid) {
  if (sid >= p->n_strings) throw Fail{GS_E_INVALID, "string id out of range"};
  if (val_of.empty()) val_of.assign(p->n_strings, kNone);
  if (val_of[sid] == kNone) val_of[sid] = value(S(sid));
  return val_of[sid];
}

uint32_t Enc::find_key(const std::string& k) const {
  if (base) {
    auto f = base->key_id.find(k);
    if (f != base->key_id.end()) return f->second;
  }
  auto f = key_id.find(k);
  return f == key_id.end() ? kNone : f->second;
}

uint32_t Enc::key_of_string(uint32_t sid) {
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

HReq Enc::make(const gs_requirement& q) {
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

HReq Enc::intersect(const HReq& a, const HReq& b) const {
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

std::map<uint32_t, HReq> Enc::reduce(gs_range rg) {
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

FList Enc::emit(const std::map<uint32_t, HReq>& m) {
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

bool Enc::has_spot(const std::map<uint32_t, HReq>& m) {
  const uint32_t k = find_key("karpenter.sh/capacity-type");
  if (k == kNone) return true;
  auto f = m.find(k);
  if (f == m.end()) return true;
  const HReq& r = f->second;
  const uint32_t v = value("spot");
  const bool in = std::binary_search(r.vals.begin(), r.vals.end(), v);
  return (r.comp ? !in : in) && within(v, r.hg, r.gt, r.hl, r.lt);
}

bool null_with_count(const gs_problem* p, bool catalog) {
  return (catalog && ((p->n_instance_types && !p->instance_types) || (p->n_offerings && !p->offerings))) ||
         (p->n_quantities && !p->quantities) || (p->n_reqs && !p->reqs) || (p->n_value_ids && !p->value_ids) ||
         (p->n_strings && !p->strings);
}

uint32_t call_column(const Enc& e, Columns& c, uint32_t sid) {
  return c.id.emplace(e.S(sid), (uint32_t)c.id.size()).first->second;
}

uint32_t resident_column(const Enc& e, Columns& c, uint32_t sid) {
  if (sid >= e.p->n_strings) throw Fail{GS_E_INVALID, "string id out of range"};
  if (c.of.empty()) c.of.assign(e.p->n_strings, kNone);
  if (c.of[sid] == kNone) {
    const std::string name = e.S(sid);
    auto f = c.catalog->id.find(name);
    c.of[sid] = f != c.catalog->id.end() ? f->second
                                         : c.catalog->R + c.id.emplace(name, (uint32_t)c.id.size()).first->second;
  }
  return c.of[sid];
}

void capacity_columns(const Enc& e, Columns& c) {
  const gs_problem* p = e.p;
  const uint32_t N = p->n_instance_types;
  e.chk(gs_range{0, N}, N, "instance_types");
  for (uint32_t i = 0; i < N; i++) {
    const gs_range cap = p->instance_types[i].capacity;
    e.chk(cap, p->n_quantities, "capacity");
    for (uint32_t k = 0; k < cap.count; k++)
      c.id.emplace(e.S(p->quantities[cap.begin + k].resource), (uint32_t)c.id.size());
  }
  c.R = std::max<uint32_t>(1, (uint32_t)c.id.size());
}

void encode_claims(Enc& e, const gs_claim_query* qs, uint32_t nq, uint32_t (*col)(const Enc&, Columns&, uint32_t),
                   Columns& c, std::vector<FQuery>& fq, std::vector<FQty>& qty) {
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
      sum[col(e, c, g.resource)] += g.milli;
    }
    x.qb = (uint32_t)qty.size();
    x.qn = (uint32_t)sum.size();
    for (auto& kv : sum) qty.push_back(FQty{kv.first, 0, kv.second});
    fq.push_back(x);
  }
}

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

}  // namespace gsf
