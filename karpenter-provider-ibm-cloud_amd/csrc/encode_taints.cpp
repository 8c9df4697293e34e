// encode_taints.cpp — the encoder's taints: the raw taint vocabulary of
// NodePools and nodes, toleration, and the taint classes the device masks carry.
#include "encode_ctx.hpp"

#include <algorithm>

namespace gsh::enc {

std::vector<uint32_t> Ctx::taint_ids(gs_range r, const std::vector<std::pair<std::string, std::string>>* reject) {
  chk(r, p->n_taints, "taints");
  std::vector<uint32_t> ids;
  for (uint32_t i = 0; i < r.count; i++) {
    auto& t = p->taints[r.begin + i];
    TaintKey tk{S(t.key), S(t.value), S(t.effect)};
    bool drop = false;
    if (reject)
      for (auto& kr : *reject) drop = drop || (kr.first == tk.k && kr.second == tk.eff);  // Taint.MatchTaint
    if (drop) continue;
    auto f = taint_id.find(tk);
    uint32_t id;
    if (f == taint_id.end()) {
      id = (uint32_t)taint_list.size();
      if (id >= (1u << 16)) throw Fail{GS_E_UNSUPPORTED, "more than 65536 distinct taints"};
      taint_id[tk] = id;
      taint_list.push_back(tk);
    } else {
      id = f->second;
    }
    ids.push_back(id);
  }
  return ids;
}

// <U> StateNode.Taints() (include/gpusched.h gs_node): while a managed node
// initializes its NodeClaim's taints stand for the node's, and its startup
// taints are ignored like the known ephemeral ones; matched by key + effect
std::vector<uint32_t> Ctx::state_taint_ids(const gs_node& g) {
  chk(g.taints, p->n_taints, "taints");
  chk(g.claim_taints, p->n_taints, "taints");
  chk(g.startup_taints, p->n_taints, "taints");
  const bool starting = g.managed && !g.initialized;
  std::vector<std::pair<std::string, std::string>> reject = {{"node.kubernetes.io/not-ready", "NoSchedule"},
                                                             {"node.kubernetes.io/unreachable", "NoSchedule"},
                                                             {"node.cloudprovider.kubernetes.io/uninitialized", "NoSchedule"},
                                                             {"karpenter.sh/unregistered", "NoExecute"}};
  if (starting)
    for (uint32_t i = 0; i < g.startup_taints.count; i++) {
      auto& t = p->taints[g.startup_taints.begin + i];
      reject.emplace_back(S(t.key), S(t.effect));
    }
  return taint_ids(starting ? g.claim_taints : g.taints, &reject);
}

// corev1 Toleration.ToleratesTaint by some toleration of the list
bool Ctx::tolerated(const std::vector<Tol>& tols, const TaintKey& tn) {
  for (auto& t : tols) {
    if (!t.eff.empty() && t.eff != tn.eff) continue;
    if (!t.k.empty() && t.k != tn.k) continue;
    if (t.op == GS_TOL_EQUAL ? t.v == tn.v : t.op == GS_TOL_EXISTS) return true;
  }
  return false;
}
// Taint classes: two taints that exactly the same spec variants tolerate are
// interchangeable in every Taints.ToleratesPod (a NodePool / node is
// tolerated iff each of its taints is), so the device masks carry one bit
// per class of equal toleration pattern; more than 64 classes is refused.
// Sets the templates' and nodes' taint masks and every variant's tol / tolt.
void Ctx::build_taint_classes() {
  const size_t NSV = variant_tols.size(), NW = (NSV + 63) / 64;
  std::map<std::vector<uint64_t>, uint32_t> cls_of;
  std::vector<uint32_t> cls(taint_list.size());
  std::vector<uint64_t> sv_tol(NSV, 0);
  std::vector<uint64_t> sig(NW);
  for (size_t id = 0; id < taint_list.size(); id++) {
    std::fill(sig.begin(), sig.end(), 0ull);
    for (size_t sv = 0; sv < NSV; sv++)
      if (tolerated(variant_tols[sv], taint_list[id])) sig[sv / 64] |= 1ull << (sv % 64);
    auto f = cls_of.find(sig);
    if (f == cls_of.end()) {
      if (cls_of.size() >= 64) throw Fail{GS_E_UNSUPPORTED, "more than 64 taint classes (distinct toleration patterns over the taints)"};
      const uint32_t c = (uint32_t)cls_of.size();
      f = cls_of.emplace(sig, c).first;
      for (size_t sv = 0; sv < NSV; sv++)
        if (sig[sv / 64] >> (sv % 64) & 1) sv_tol[sv] |= 1ull << c;
    }
    cls[id] = f->second;
  }
  auto mask = [&](const std::vector<uint32_t>& ids) {
    uint64_t m = 0;
    for (uint32_t id : ids) m |= 1ull << cls[id];
    return m;
  };
  for (uint32_t t = 0; t < e.T; t++) e.tmpl[t].taints = mask(tmpl_taints[t]);
  e.tmpl_taint_order.assign(e.T, {});
  for (uint32_t t = 0; t < e.T; t++) {
    // taint_ids kept every taint of the NodePool (no reject list): position i is taints.begin + i
    const uint32_t begin = p->nodepools[e.tmpl[t].np_index].taints.begin;
    for (uint32_t i = 0; i < tmpl_taints[t].size(); i++)
      e.tmpl_taint_order[t].emplace_back(begin + i, cls[tmpl_taints[t][i]]);
  }
  for (uint32_t pos = 0; pos < e.NN; pos++) e.nodes[pos].taints = mask(node_taints[pos]);
  for (uint32_t v = 0; v < e.V; v++) {
    gsd::VarRec& vr = e.vars[v];
    vr.tol = sv_tol[e.var_sv[v]];
    vr.tolt = 0;
    for (uint32_t t = 0; t < e.T; t++)
      if ((e.tmpl[t].taints & ~vr.tol) == 0) vr.tolt |= 1ull << t;
  }
  for (size_t sv = 0; sv < NSV; sv++) e.variants[sv].tol = sv_tol[sv];
  final_sv_tol = std::move(sv_tol);
  taint_cls = cls;
}

}  // namespace gsh::enc
