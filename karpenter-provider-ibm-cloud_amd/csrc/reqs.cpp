// reqs.cpp — the requirement algebra on vocabulary bitsets (encode.hpp): a
// restatement of <U> sigs.k8s.io/karpenter pkg/scheduling (Requirement.
// Intersection/Has/Len/Operator, Requirements.Compatible/Intersects),
// independent of the oracle's string-set one (oracle/solve.cpp); and the label
// helpers the encoder, decode and the launch-time re-filter (filter.hip) share.
#include "encode.hpp"

#include <algorithm>
#include <climits>
#include <set>

namespace gsh {

// <U> v1.WellKnownLabels + IBM keys (reference pkg/apis/v1alpha1/labels.go:37-45)
bool label_is_wellknown(const std::string& k) {
  static const std::set<std::string> s = {
      "karpenter.sh/nodepool",           "topology.kubernetes.io/zone",      "topology.kubernetes.io/region",
      "node.kubernetes.io/instance-type", "kubernetes.io/arch",              "kubernetes.io/os",
      "karpenter.sh/capacity-type",       "node.kubernetes.io/windows-build", "karpenter-ibm.sh/instance-size",
      "karpenter-ibm.sh/instance-family", "karpenter-ibm.sh/instance-cpu",   "karpenter-ibm.sh/instance-memory"};
  return s.count(k) != 0;
}

std::string label_normalize(const std::string& k) {
  if (k == "failure-domain.beta.kubernetes.io/zone") return "topology.kubernetes.io/zone";
  if (k == "failure-domain.beta.kubernetes.io/region") return "topology.kubernetes.io/region";
  if (k == "beta.kubernetes.io/arch") return "kubernetes.io/arch";
  if (k == "beta.kubernetes.io/instance-type") return "node.kubernetes.io/instance-type";
  if (k == "beta.kubernetes.io/os") return "kubernetes.io/os";
  return k;
}

// strconv.Atoi
bool go_atoi64(const std::string& s, int64_t* out) {
  if (s.empty()) return false;
  size_t i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    i = 1;
  }
  if (i == s.size()) return false;
  unsigned __int128 v = 0;
  for (; i < s.size(); i++) {
    if (s[i] < '0' || s[i] > '9') return false;
    v = v * 10 + (unsigned)(s[i] - '0');
    if (v > (unsigned __int128)INT64_MAX + 1) return false;
  }
  if (!neg && v > (unsigned __int128)INT64_MAX) return false;
  *out = neg ? (int64_t)(-(__int128)v) : (int64_t)v;
  return true;
}

Bits within_mask(const Vocab& v, bool hg, int64_t gt, bool hl, int64_t lt) {
  Bits b(v.words());
  for (size_t i = 0; i < v.size(); i++) {
    if (!hg && !hl) {
      b.set(i);
      continue;
    }
    if (!v.isint[i]) continue;
    if (hg && gt >= v.ival[i]) continue;
    if (hl && lt <= v.ival[i]) continue;
    b.set(i);
  }
  return b;
}

static Bits all_bits(const Vocab& v) { return within_mask(v, false, 0, false, 0); }

KReq kreq_intersect(const Vocab& v, const KReq& a, const KReq& b) {
  KReq r;
  r.comp = a.comp && b.comp;
  r.hg = a.hg || b.hg;
  r.gt = a.hg && b.hg ? std::max(a.gt, b.gt) : (a.hg ? a.gt : b.gt);
  r.hl = a.hl || b.hl;
  r.lt = a.hl && b.hl ? std::min(a.lt, b.lt) : (a.hl ? a.lt : b.lt);
  r.mv = std::max(a.mv, b.mv);
  if (r.hg && r.hl && r.gt >= r.lt) {  // DoesNotExist
    KReq d;
    d.comp = false;
    d.has = Bits(v.words());
    d.excl = Bits(v.words());
    d.mv = r.mv;
    return d;
  }
  r.has = a.has;
  r.has &= b.has;
  r.excl = Bits(v.words());
  if (r.comp) {
    r.excl = a.excl;
    r.excl |= b.excl;
    r.excl &= within_mask(v, r.hg, r.gt, r.hl, r.lt);
  } else {
    r.hg = r.hl = false;
    r.gt = r.lt = 0;
  }
  return r;
}

KReq make_kreq(const Vocab& v, int op, const std::vector<uint32_t>& vals, int64_t bound) {
  KReq q;
  q.has = Bits(v.words());
  q.excl = Bits(v.words());
  switch (op) {
    case GS_OP_IN:
      q.comp = false;
      for (auto x : vals) q.has.set(x);
      break;
    case GS_OP_NOTIN:
      q.comp = true;
      for (auto x : vals) q.excl.set(x);
      q.has = all_bits(v);
      for (auto x : vals) q.has.reset(x);
      break;
    case GS_OP_EXISTS:
      q.comp = true;
      q.has = all_bits(v);
      break;
    case GS_OP_DOES_NOT_EXIST:
      q.comp = false;
      break;
    case GS_OP_GT:
      q.comp = true;
      q.hg = true;
      q.gt = bound;
      q.has = within_mask(v, true, bound, false, 0);
      break;
    case GS_OP_LT:
      q.comp = true;
      q.hl = true;
      q.lt = bound;
      q.has = within_mask(v, false, 0, true, bound);
      break;
  }
  return q;
}

void reqs_add(const Encoded& e, Reqs& r, uint32_t key, const KReq& q) {
  auto it = r.find(key);
  if (it == r.end()) r.emplace(key, q);
  else it->second = kreq_intersect(e.keys[key].vocab, q, it->second);
}

void reqs_add_all(const Encoded& e, Reqs& r, const Reqs& o) {
  for (auto& kv : o) reqs_add(e, r, kv.first, kv.second);
}

bool reqs_compatible(const Encoded& e, const Reqs& r, const Reqs& in, bool allow_wk) {
  for (auto& kv : in) {
    if (allow_wk && e.keys[kv.first].wellknown) continue;
    if (r.count(kv.first)) continue;
    if (exempt(kv.second)) continue;
    return false;
  }
  for (auto& kv : in) {
    auto it = r.find(kv.first);
    if (it == r.end()) continue;
    KReq x = kreq_intersect(e.keys[kv.first].vocab, it->second, kv.second);
    if (len_zero(x) && !(exempt(it->second) && exempt(kv.second))) return false;
  }
  return true;
}

std::string canonical(const Encoded& e, const Reqs& r) {
  std::vector<std::pair<std::string, const KReq*>> items;
  for (auto& kv : r) items.push_back({e.keys[kv.first].name, &kv.second});
  std::sort(items.begin(), items.end(), [](auto& a, auto& b) { return a.first < b.first; });
  static const char* opn[] = {"In", "NotIn", "Exists", "DoesNotExist"};
  std::string s;
  for (auto& it : items) {
    const KReq& q = *it.second;
    const Vocab& v = e.keys[e.key_id.at(it.first)].vocab;
    if (!s.empty()) s += '\n';
    s += it.first;
    s += '|';
    s += opn[op_of(q)];
    s += '|';
    std::vector<std::string> vals;
    const Bits& b = q.comp ? q.excl : q.has;
    for (size_t i = 0; i < v.size(); i++)
      if (b.test(i)) vals.push_back(v.vals[i]);
    std::sort(vals.begin(), vals.end());
    for (size_t i = 0; i < vals.size(); i++) {
      if (i) s += ',';
      s += vals[i];
    }
    s += '|';
    s += q.comp && q.hg ? std::to_string(q.gt) : "-";
    s += '|';
    s += q.comp && q.hl ? std::to_string(q.lt) : "-";
    s += '|';
    s += q.mv >= 0 ? std::to_string(q.mv) : "-";
  }
  return s;
}

}  // namespace gsh
