// encode_pods.cpp — the encoder's pod phase: pods -> specs, topology group
// ids, Relax variants, the device variant records and the queue order.
#include "encode_ctx.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace gsh::enc {

// A pod's spec as bytes: everything but its uid, creation time, requests
// and volumes (canonical string ids, so equal text is equal bytes).  Pods
// with equal bytes have the same variants, groups and selection lists
// (Deployments: thousands of replicas, one spec).  false: a range or id is
// out of bounds (the pod is its own spec; its encode raises the error).
bool Ctx::pod_sig(const gs_pod& pd, std::vector<uint32_t>& out) const {
  auto u32 = [&](uint32_t x) { out.push_back(x); };
  auto sid = [&](uint32_t id) {
    if (id >= canon.size()) return false;
    u32(canon[id]);
    return true;
  };
  auto rng = [&](gs_range r, uint32_t n) { return (uint64_t)r.begin + r.count <= n; };
  auto labels = [&](gs_range r) {
    if (!rng(r, p->n_labels)) return false;
    u32(r.count);
    for (uint32_t k = 0; k < r.count; k++)
      if (!sid(p->labels[r.begin + k].key) || !sid(p->labels[r.begin + k].value)) return false;
    return true;
  };
  auto vids = [&](gs_range r) {
    if (!rng(r, p->n_value_ids)) return false;
    u32(r.count);
    for (uint32_t k = 0; k < r.count; k++)
      if (!sid(p->value_ids[r.begin + k])) return false;
    return true;
  };
  auto reqs = [&](gs_range r) {
    if (!rng(r, p->n_reqs)) return false;
    u32(r.count);
    for (uint32_t k = 0; k < r.count; k++) {
      const gs_requirement& q = p->reqs[r.begin + k];
      if (!sid(q.key)) return false;
      u32(q.op);
      u32((uint32_t)q.min_values);
      if (!vids(q.values)) return false;
    }
    return true;
  };
  auto terms = [&](gs_range r) {
    if (!rng(r, p->n_terms)) return false;
    u32(r.count);
    for (uint32_t k = 0; k < r.count; k++) {
      u32((uint32_t)p->terms[r.begin + k].weight);
      if (!reqs(p->terms[r.begin + k].requirements)) return false;
    }
    return true;
  };
  auto aff = [&](gs_range r) {
    if (!rng(r, p->n_affinity_terms)) return false;
    u32(r.count);
    for (uint32_t k = 0; k < r.count; k++) {
      const gs_affinity_term& q = p->affinity_terms[r.begin + k];
      if (!sid(q.topology_key)) return false;
      u32(q.required);
      u32((uint32_t)q.weight);
      u32(q.has_selector);
      u32(q.has_ns_selector);
      if (!labels(q.match_labels) || !reqs(q.match_expressions) || !vids(q.namespaces) ||
          !labels(q.ns_match_labels) || !reqs(q.ns_match_expressions))
        return false;
    }
    return true;
  };
  out.clear();
  u32(pd.flags);
  if (!sid(pd.ns) || !labels(pd.node_selector) || !terms(pd.required_terms) || !terms(pd.preferred_terms) ||
      !labels(pd.labels) || !rng(pd.tolerations, p->n_tolerations) || !rng(pd.spreads, p->n_spreads) ||
      !rng(pd.host_ports, p->n_host_ports))
    return false;
  u32(pd.tolerations.count);
  for (uint32_t k = 0; k < pd.tolerations.count; k++) {
    const gs_toleration& t = p->tolerations[pd.tolerations.begin + k];
    u32(t.op);
    if (!sid(t.key) || !sid(t.value) || !sid(t.effect)) return false;
  }
  u32(pd.spreads.count);
  for (uint32_t k = 0; k < pd.spreads.count; k++) {
    const gs_spread& q = p->spreads[pd.spreads.begin + k];
    if (!sid(q.topology_key)) return false;
    u32((uint32_t)q.max_skew);
    u32(q.when_unsatisfiable);
    u32((uint32_t)q.min_domains);
    u32(q.has_selector);
    u32(q.node_affinity_policy);
    u32(q.node_taints_policy);
    if (!labels(q.match_labels) || !reqs(q.match_expressions) || !vids(q.match_label_keys)) return false;
  }
  if (!aff(pd.anti_affinity) || !aff(pd.affinity)) return false;
  u32(pd.host_ports.count);
  for (uint32_t k = 0; k < pd.host_ports.count; k++) {
    const gs_host_port& h = p->host_ports[pd.host_ports.begin + k];
    u32((uint32_t)h.port);
    if (!sid(h.protocol) || !sid(h.ip)) return false;
  }
  return true;
}

// Per-spec encode work.  Phase A (parallel over specs) builds everything
// the spec determines; phase B (serial, in the order pods first carry each
// spec) assigns topology group ids, numbered in the order pods first name
// them; phase C (parallel) builds the Relax variants.  An error is the
// serial encoder's: the first failing pod's.
struct GroupKey {
  std::string key;
  GroupEnc g;
  bool required = false;
  int32_t weight = 0;
};
struct PodWork {
  Reqs ns;
  std::vector<Reqs> req_terms;
  std::vector<std::pair<int32_t, Reqs>> pref;
  std::vector<SpreadEnc> sps;
  std::vector<std::string> sp_hash, sp_merge;
  std::vector<GroupKey> g_anti, g_aff, g_inv, g_port;  // in the order the pod names them
  std::vector<Tol> tols;
  std::vector<uint32_t> sgid, own_static;
  std::vector<std::pair<int32_t, uint32_t>> anti_pref, aff_pref;  // (weight, group)
  std::vector<PodVariant> vars;
  std::vector<std::vector<Tol>> var_tols;
  std::string aff_text;             // the node filter's terms with their values
  std::vector<uint32_t> pref_keys;  // keys of the preferred node-affinity terms
  // relaxation states of the spreads' node filter (<U> MakeTopologyNodeFilter
  // of the relaxed pod): state r < nT keeps the required terms from r on,
  // state nT adds the PreferNoSchedule toleration; per state the spreads
  // as that pod would key them, their hashes and group ids
  uint32_t n_states = 1;
  std::vector<std::vector<SpreadEnc>> st_sps;
  std::vector<std::vector<std::string>> st_hash;
  std::vector<std::vector<uint32_t>> st_gid;
  std::vector<uint32_t> var_state;  // per variant
};
// <U> MakeTopologyNodeFilter of one relaxation state: node selector AND
// each required term from ri on (the selector alone without terms), the
// tolerations; fid = TopologyGroup.Hash's part (term keys, tolerations),
// text = the terms with their values, zone_only = no key past the zone
struct FilterState {
  std::vector<Reqs> fr;
  std::string fid, text;
  bool zone_only = true, empty = true;
};

FilterState Ctx::filter_state(const PodWork& w, size_t ri, const std::vector<Tol>& tols) const {
  FilterState f;
  if (w.req_terms.empty()) f.fr.push_back(w.ns);
  for (size_t t = ri; t < w.req_terms.size(); t++) {
    Reqs r = w.ns;
    for (auto& kv : w.req_terms[t]) reqs_add(e, r, kv.first, kv.second);
    f.fr.push_back(std::move(r));
  }
  std::vector<std::string> texts, terms, tl;
  for (auto& r : f.fr) {
    texts.push_back(canonical(e, r));
    std::vector<std::string> ks;
    for (auto& kv : r) ks.push_back(e.keys[kv.first].name);
    std::sort(ks.begin(), ks.end());
    std::string k;
    for (auto& x : ks) k += x + ",";
    terms.push_back(std::move(k));
    f.empty = f.empty && r.empty();
  }
  std::sort(texts.begin(), texts.end());
  for (auto& t : texts) f.text += t + "\x1e";
  for (auto& t : tols) tl.push_back(t.k + "=" + t.v + ":" + t.eff + "/" + std::to_string(t.op));
  std::sort(terms.begin(), terms.end());
  std::sort(tl.begin(), tl.end());
  for (auto& t : terms) f.fid += t + ";";
  f.fid += "#";
  for (auto& t : tl) f.fid += t + ";";
  for (auto& kv : w.ns) f.zone_only = f.zone_only && kv.first == e.k_zone;
  for (size_t t = ri; t < w.req_terms.size(); t++)
    for (auto& kv : w.req_terms[t]) f.zone_only = f.zone_only && kv.first == e.k_zone;
  return f;
}
// the spreads keyed under one filter state.  nodeAffinityPolicy Honor
// equals Ignore when the filter constrains the zone key alone
// (oracle/solve.cpp: it then drops only nodes / NodeClaims outside the
// owner's zones); other filters are applied exactly where they can differ:
// a bound pod counts only on a node the filter matches, and the pending
// pods the group counts must carry the owner's filter terms
// (build_topology), so every NodeClaim / node they land on matches it
static void key_spreads(std::vector<SpreadEnc>& sps, const FilterState& f) {
  for (auto& sp : sps) {
    sp.fid = f.fid;
    sp.ftext = sp.ignore_aff ? std::string() : f.text;
    sp.strict_aff = !f.zone_only && !sp.ignore_aff;
    sp.filter = sp.strict_aff ? f.fr : std::vector<Reqs>();
  }
}

void Ctx::pod_phase_a(uint32_t i, PodWork& w, const std::map<std::string, AntiEnc>& inv_terms) {
  const bool topo_inputs = this->topo_inputs();
  auto& pd = p->pods[i];
  w.ns = labels_reqs(pd.node_selector);
  for (uint32_t k = 0; k < pd.required_terms.count; k++) {
    no_min_values(p->terms[pd.required_terms.begin + k].requirements);
    w.req_terms.push_back(reqs_of(p->terms[pd.required_terms.begin + k].requirements));
  }
  for (uint32_t k = 0; k < pd.preferred_terms.count; k++) {
    auto& tm = p->terms[pd.preferred_terms.begin + k];
    no_min_values(tm.requirements);
    w.pref.push_back({tm.weight, reqs_of(tm.requirements)});
  }
  if (w.pref.size() > 12) throw Fail{GS_E_UNSUPPORTED, "more than 12 preferred node-affinity terms"};
  // sort.Slice by weight desc on <= 12 elements is insertion sort: stable
  std::stable_sort(w.pref.begin(), w.pref.end(), [](auto& a, auto& b) { return a.first > b.first; });
  // topology spread constraints -> groups (owners); namespace / labels for selectors
  const std::string& pns = S(pd.ns);
  chk(pd.labels, p->n_labels, "labels");
  w.sps = spreads_of(pd);
  chk(pd.tolerations, p->n_tolerations, "tolerations");
  for (uint32_t k = 0; k < pd.tolerations.count; k++) {
    auto& t = p->tolerations[pd.tolerations.begin + k];
    w.tols.push_back({S(t.key), S(t.value), S(t.effect), t.op});
  }
  // <U> MakeTopologyNodeFilter: node selector AND each required term.  Its
  // text (terms with values) is kept for every spec of a problem with
  // topology inputs: a spec counted by a group whose Honor filter reaches
  // past the zone key must carry that same filter (build_topology)
  FilterState f0;
  if (topo_inputs || !w.sps.empty()) f0 = filter_state(w, 0, w.tols);
  if (topo_inputs) {
    w.aff_text = f0.text;
    for (auto& pr : w.pref)
      for (auto& kv : pr.second) w.pref_keys.push_back(kv.first);
  }
  if (!w.sps.empty()) {
    key_spreads(w.sps, f0);
    // the states Relax moves the filter through: each dropped required
    // term, then the PreferNoSchedule toleration (pod_phase_c's order)
    const size_t nT = std::max<size_t>(w.req_terms.size(), 1);
    bool has_pns = false;
    for (auto& t : w.tols) has_pns = has_pns || (t.k.empty() && t.op == GS_TOL_EXISTS && t.v.empty() && t.eff == kPNS);
    w.n_states = (uint32_t)nT + (tolerate_pns && !has_pns ? 1u : 0u);
    w.st_sps.resize(w.n_states);
    w.st_hash.resize(w.n_states);
    w.st_gid.resize(w.n_states);
    for (uint32_t st = 1; st < w.n_states; st++) {
      std::vector<Tol> tols = w.tols;
      if (st == nT) tols.push_back({"", "", kPNS, GS_TOL_EXISTS});
      w.st_sps[st] = w.sps;
      key_spreads(w.st_sps[st], filter_state(w, std::min<size_t>(st, nT - 1), tols));
      for (auto& sp : w.st_sps[st]) w.st_hash[st].push_back(sp.hash(pns));
    }
  }
  const bool filter_empty = f0.empty;
  for (auto& sp : w.sps) {
    w.sp_hash.push_back(sp.hash(pns));
    std::string mk;
    // GS_GROUP_MERGE=0: one group per upstream group (A/B knob)
    static const bool merge_on = !std::getenv("GS_GROUP_MERGE") || std::atoi(std::getenv("GS_GROUP_MERGE")) != 0;
    if (merge_on && !sp.honor_taints && (sp.ignore_aff || filter_empty)) {
      SpreadEnc x = sp;
      x.fid = "-";
      mk = x.hash(pns) + "|m:" + std::to_string(sp.mind);
    }
    w.sp_merge.push_back(std::move(mk));
  }
  // anti-affinity, inverse anti-affinity and host-port groups
  if (topo_inputs) {
    const PodSel& me = pod_sel[spec_of[i]];
    for (auto& a : antis_of(pd)) {
      const bool self = a.selects(me.ns, me.labels);
      GroupEnc g = host_group(1, self, a.sel.key);
      g.anti = a;
      w.g_anti.push_back(GroupKey{"A|" + a.hash() + (self ? "|s" : "|n"), std::move(g), a.required, a.weight});
    }
    for (auto& a : terms_of(pd, pd.affinity, true)) {
      GroupEnc g = host_group(4, false);
      g.anti = a;
      w.g_aff.push_back(GroupKey{"F|" + a.hash(), std::move(g), a.required, a.weight});
    }
    for (auto& kv : inv_terms) {
      if (!kv.second.selects(me.ns, me.labels)) continue;
      const bool self = me.carried.count(kv.first) != 0;
      GroupEnc g = host_group(2, self, kv.second.sel.key);
      g.inv_hash = kv.first;
      w.g_inv.push_back(GroupKey{"I|" + kv.first + (self ? "|s" : "|n"), std::move(g)});
    }
    for (auto& pe : me.ports) {
      GroupEnc g = host_group(3, true);
      g.port = pe;
      w.g_port.push_back(GroupKey{"P|" + pe.key(), std::move(g)});
    }
  }
}

void Ctx::pod_phase_b(uint32_t i, PodWork& w) {
  const std::string pns = S(p->pods[i].ns);
  for (size_t k = 0; k < w.sps.size(); k++) {
    auto f = group_idx.find(w.sp_hash[k]);
    if (f == group_idx.end()) {
      auto m = w.sp_merge[k].empty() ? merge_idx.end() : merge_idx.find(w.sp_merge[k]);
      if (m != merge_idx.end()) {
        f = group_idx.emplace(w.sp_hash[k], m->second).first;
      } else {
        if (groups.size() >= (size_t)gsd::TGMAX) throw Fail{GS_E_UNSUPPORTED, "more than 4096 topology groups"};
        f = group_idx.emplace(w.sp_hash[k], (uint32_t)groups.size()).first;
        if (!w.sp_merge[k].empty()) merge_idx.emplace(w.sp_merge[k], (uint32_t)groups.size());
        groups.push_back(GroupEnc{w.sps[k], pns});
        groups.back().owner_spec = spec_of[i];
      }
    } else if (!w.sps[k].ignore_aff && groups[f->second].sp.ftext != w.sps[k].ftext) {
      // upstream keys the group by the filter's keys and keeps its first
      // owner's filter: later owners with other values would see counts
      // filtered by someone else's node affinity
      throw Fail{GS_E_UNSUPPORTED,
                 "pods sharing a topology spread (nodeAffinityPolicy Honor) with different node affinity values"};
    }
    w.sgid.push_back(f->second);
  }
  for (auto& gk : w.g_anti) {
    const uint32_t gid = group_id(gk.key, std::move(gk.g));
    if (gk.required) w.own_static.push_back(gid);
    else w.anti_pref.push_back({gk.weight, gid});
  }
  if (w.anti_pref.size() > 12) throw Fail{GS_E_UNSUPPORTED, "more than 12 preferred anti-affinity terms"};
  for (auto& gk : w.g_aff) {
    const uint32_t gid = group_id(gk.key, std::move(gk.g));
    if (gk.required) w.own_static.push_back(gid);
    else w.aff_pref.push_back({gk.weight, gid});
  }
  if (w.aff_pref.size() > 12) throw Fail{GS_E_UNSUPPORTED, "more than 12 preferred pod affinity terms"};
  // sort.Slice by weight desc on <= 12 elements is insertion sort: stable
  std::stable_sort(w.aff_pref.begin(), w.aff_pref.end(), [](auto& a, auto& b) { return a.first > b.first; });
  std::stable_sort(w.anti_pref.begin(), w.anti_pref.end(), [](auto& a, auto& b) { return a.first > b.first; });
  for (auto& gk : w.g_inv) w.own_static.push_back(group_id(gk.key, std::move(gk.g)));
  for (auto& gk : w.g_port) w.own_static.push_back(group_id(gk.key, std::move(gk.g)));
  // the first variant owns every group (later ones only drop groups)
  std::vector<uint32_t> own = w.sgid;
  own.insert(own.end(), w.own_static.begin(), w.own_static.end());
  for (auto& x : w.anti_pref) own.push_back(x.second);
  for (auto& x : w.aff_pref) own.push_back(x.second);
  std::sort(own.begin(), own.end());
  if (std::unique(own.begin(), own.end()) - own.begin() > (ptrdiff_t)gsd::OWNMAX)
    throw Fail{GS_E_UNSUPPORTED, "a pod owns more than 64 topology groups"};
  w.g_anti.clear();
  w.g_aff.clear();
  w.g_inv.clear();
  w.g_port.clear();
}

void Ctx::pod_phase_b2(uint32_t s, PodWork& w) {
  const std::string pns = S(p->pods[spec_rep[s]].ns);
  for (uint32_t st = 1; st < w.n_states; st++) {
    w.st_gid[st].clear();
    for (size_t k = 0; k < w.st_sps[st].size(); k++) {
      const SpreadEnc& sp = w.st_sps[st][k];
      auto f = group_idx.find(w.st_hash[st][k]);
      if (f == group_idx.end()) {
        // Topology.Update's new group counts the cluster's bound pods only
        // (a hostname group also lacks the in-flight NodeClaims registered
        // before it: the kernels mark those HC_UNKNOWN when it is created)
        if (groups.size() >= (size_t)gsd::TGMAX) throw Fail{GS_E_UNSUPPORTED, "more than 4096 topology groups"};
        if (n_lazy >= (uint32_t)gsd::TGMAX)
          throw Fail{GS_E_UNSUPPORTED, "more than 4096 topology spread groups created by relaxation"};
        f = group_idx.emplace(w.st_hash[st][k], (uint32_t)groups.size()).first;
        groups.push_back(GroupEnc{sp, pns});
        GroupEnc& g = groups.back();
        g.owner_spec = s;
        g.lazy = true;
        g.lazy_idx = n_lazy++;
        g.owner_state = st;
      } else {
        const GroupEnc& g = groups[f->second];
        if (!sp.ignore_aff && g.sp.ftext != sp.ftext)
          throw Fail{GS_E_UNSUPPORTED,
                     "pods sharing a topology spread (nodeAffinityPolicy Honor) with different node affinity values"};
      }
      w.st_gid[st].push_back(f->second);
    }
  }
}

// <U> NewPodRequirements + Preferences.Relax: every variant of one spec
void Ctx::pod_phase_c(PodWork& w) {
  std::vector<uint32_t> cur(w.sps.size());  // current constraints (swap-remove order)
  std::iota(cur.begin(), cur.end(), 0);
  std::vector<Tol> tols = w.tols;
  size_t ri = 0, pi = 0, ai = 0, fi = 0;
  uint32_t state = 0;  // the spreads' filter state (pod_phase_a)
  if (!w.sps.empty()) w.st_gid[0] = w.sgid;
  for (;;) {
    // <U> NewPodRequirements: nodeSelector + heaviest preferred + first required
    PodVariant v;
    v.reqs = w.ns;
    v.strict = w.ns;
    if (pi < w.pref.size()) reqs_add_all(e, v.reqs, w.pref[pi].second);
    if (ri < w.req_terms.size()) {
      reqs_add_all(e, v.reqs, w.req_terms[ri]);
      reqs_add_all(e, v.strict, w.req_terms[ri]);
    }
    v.tol = 0;  // build_taint_classes
    for (uint32_t k : cur) {
      const uint32_t g = w.st_gid[state][k];
      v.own.push_back(g);
      // the pod that relaxes first creates a lazy group with its own
      // minDomains (the kernels set it at that Relax)
      if (groups[g].lazy) v.lazy_mind.emplace_back(groups[g].lazy_idx, w.st_sps[state][k].mind);
    }
    w.var_state.push_back(state);
    v.own.insert(v.own.end(), w.own_static.begin(), w.own_static.end());
    for (size_t k = ai; k < w.anti_pref.size(); k++) v.own.push_back(w.anti_pref[k].second);
    for (size_t k = fi; k < w.aff_pref.size(); k++) v.own.push_back(w.aff_pref[k].second);
    std::sort(v.own.begin(), v.own.end());
    v.own.erase(std::unique(v.own.begin(), v.own.end()), v.own.end());
    w.vars.push_back(std::move(v));
    w.var_tols.push_back(tols);
    // <U> Preferences.Relax
    if (w.req_terms.size() - ri > 1) {
      ri++;
      state = (uint32_t)ri;
      continue;
    }
    // removePreferredPodAffinityTerm, then ...AntiAffinityTerm (the heaviest)
    if (fi < w.aff_pref.size()) {
      fi++;
      continue;
    }
    if (ai < w.anti_pref.size()) {
      ai++;
      continue;
    }
    if (pi < w.pref.size()) {
      pi++;
      continue;
    }
    // removeTopologySpreadScheduleAnyway: swap-remove the first one
    bool removed = false;
    for (size_t k = 0; k < cur.size() && !removed; k++)
      if (w.sps[cur[k]].sa) {
        cur[k] = cur.back();
        cur.pop_back();
        removed = true;
      }
    if (removed) continue;
    if (tolerate_pns) {
      bool has = false;
      for (auto& t : tols)
        if (t.k.empty() && t.op == GS_TOL_EXISTS && t.v.empty() && t.eff == kPNS) has = true;
      if (!has) {
        tols.push_back({"", "", kPNS, GS_TOL_EXISTS});
        state = w.n_states - 1;
        continue;
      }
    }
    break;
  }
}

void Ctx::build_pods() {
  e.P = p->n_pods;
  e.pod_req.assign((size_t)e.P * e.R, 0);
  pod_specs();
  tm.sub("specs");
  const std::map<std::string, AntiEnc> inv_terms = pod_inverse_terms();
  tm.sub("groups");
  const std::pair<uint32_t, bool> dup = pod_dup_uid();
  tm.sub("uids");
  std::vector<PodWork> work = pod_spec_work(inv_terms, dup);
  tm.sub("spec_work");
  pod_variants(std::move(work));
  tm.sub("variants");
  pod_var_records();
  tm.sub("var_records");
  pod_queue_order();
  tm.sub("queue_sort");
  e.checks = (uint64_t)e.P * e.checks_per_pod;
}

// pods -> specs (first-carrier order): a 64-bit hash of each pod's spec
// bytes in parallel, specs numbered by first hash occurrence, then every
// pod's bytes compared with its spec's first pod's (a hash collision
// falls back to an exact map over the bytes)
void Ctx::pod_specs() {
  spec_of.assign(e.P, 0);
  spec_rep.clear();
  auto mix = [](const std::vector<uint32_t>& v) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ v.size();
    for (uint32_t x : v) {
      h ^= x;
      h *= 0xFF51AFD7ED558CCDull;
      h ^= h >> 32;
    }
    return h;
  };
  std::vector<uint64_t> hs(e.P);
  std::vector<uint8_t> ok(e.P, 0);
  par_for(e.P, 1024, [&](uint32_t i) {
    thread_local std::vector<uint32_t> buf;
    buf.clear();
    ok[i] = pod_sig(p->pods[i], buf);
    hs[i] = mix(buf);
  });
  std::unordered_map<uint64_t, uint32_t> first;
  first.reserve(256);
  for (uint32_t i = 0; i < e.P; i++) {
    if (!ok[i]) {
      spec_of[i] = (uint32_t)spec_rep.size();
      spec_rep.push_back(i);
      continue;
    }
    auto f = first.emplace(hs[i], (uint32_t)spec_rep.size());
    if (f.second) spec_rep.push_back(i);
    spec_of[i] = f.first->second;
  }
  std::vector<uint8_t> clash(e.P, 0);
  par_for(e.P, 1024, [&](uint32_t i) {
    const uint32_t r = spec_rep[spec_of[i]];
    if (r == i) return;
    thread_local std::vector<uint32_t> a, b;
    a.clear();
    b.clear();
    pod_sig(p->pods[i], a);
    pod_sig(p->pods[r], b);
    clash[i] = a != b;
  });
  std::map<std::vector<uint32_t>, uint32_t> exact;  // specs a collision split off
  for (uint32_t i = 0; i < e.P; i++) {
    if (!clash[i]) continue;
    std::vector<uint32_t> a;
    pod_sig(p->pods[i], a);
    auto f = exact.emplace(std::move(a), (uint32_t)spec_rep.size());
    if (f.second) spec_rep.push_back(i);
    spec_of[i] = f.first->second;
  }
  // specs numbered in first-carrier order (a collision's spec was appended)
  std::vector<uint32_t> order(spec_rep.size());
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return spec_rep[x] < spec_rep[y]; });
  std::vector<uint32_t> rank(spec_rep.size());
  for (uint32_t k = 0; k < order.size(); k++) rank[order[k]] = k;
  std::vector<uint32_t> rep2(spec_rep.size());
  for (uint32_t k = 0; k < order.size(); k++) rep2[k] = spec_rep[order[k]];
  spec_rep.swap(rep2);
  for (uint32_t i = 0; i < e.P; i++) spec_of[i] = rank[spec_of[i]];
}

// <U> the inverse anti-affinity groups: required terms of pending and
// bound pods (Topology.updateInverseAntiAffinity / updateInverseAffinities);
// and what makes each spec's pods counted by a group (pod_sel)
std::map<std::string, AntiEnc> Ctx::pod_inverse_terms() {
  const uint32_t NS = (uint32_t)spec_rep.size();
  std::map<std::string, AntiEnc> inv_terms;
  if (topo_inputs()) {
    pod_sel.assign(NS, PodSel{});
    std::vector<std::vector<AntiEnc>> req_antis(NS);
    par_try(NS, 8, [&](uint32_t s) {
      pod_sel[s] = sel_of(p->pods[spec_rep[s]]);
      for (auto& a : antis_of(p->pods[spec_rep[s]]))
        if (a.required) req_antis[s].push_back(std::move(a));
    }).rethrow();
    // specs in first-carrier order: the first-inserted term is the serial encoder's
    for (uint32_t s = 0; s < NS; s++)
      for (auto& a : req_antis[s]) inv_terms.emplace(a.hash(), a);
    chk(gs_range{0, p->n_bound_pods}, p->n_bound_pods, "bound pods");
    for (uint32_t b = 0; b < p->n_bound_pods; b++)
      for (auto& a : antis_of(p->bound_pods[b]))
        if (a.required) inv_terms.emplace(a.hash(), a);
  } else {
    for (uint32_t i = 0; i < e.P; i++) {
      chk(p->pods[i].anti_affinity, p->n_affinity_terms, "affinity_terms");
      chk(p->pods[i].affinity, p->n_affinity_terms, "affinity_terms");
      chk(p->pods[i].host_ports, p->n_host_ports, "host_ports");
    }
  }
  return inv_terms;
}

// the first pod whose uid an earlier pod carries, or names no string (second:
// which of the two; first = P: none)
std::pair<uint32_t, bool> Ctx::pod_dup_uid() const {
  std::vector<uint8_t> uid_seen(strs.size(), 0);
  for (uint32_t i = 0; i < e.P; i++) {
    if (p->pods[i].uid >= canon.size()) return {i, true};
    const uint32_t cu = canon[p->pods[i].uid];
    if (uid_seen[cu]) return {i, false};
    uid_seen[cu] = 1;
  }
  return {e.P, false};
}

// requests per pod, the spec's work per spec (pod_phase_a .. pod_phase_c).  An
// error is the first failing pod's; on one pod its flags come first, then its
// uid (dup), then its requests, then its spec's work
std::vector<PodWork> Ctx::pod_spec_work(const std::map<std::string, AntiEnc>& inv_terms, std::pair<uint32_t, bool> dup) {
  const uint32_t NS = (uint32_t)spec_rep.size(), dup_at = dup.first;
  const ParErr rerr = par_try(e.P, 1024, [&](uint32_t i) {
    resvec_fn(p->pods[i].requests, &e.pod_req[(size_t)i * e.R], nullptr);
  });
  std::vector<PodWork> work(NS);
  const ParErr aerr = par_try(NS, 8, [&](uint32_t s) {
    const uint32_t i = spec_rep[s];
    if (p->pods[i].flags || i >= dup_at) return;
    pod_phase_a(i, work[s], inv_terms);
  });
  for (uint32_t i = 0; i < e.P; i++) {
    if (p->pods[i].flags) throw Fail{GS_E_UNSUPPORTED, "pod topology spread / pod affinity / host ports / volumes"};
    if (i == dup_at) throw Fail{GS_E_INVALID, dup.second ? "string id out of range" : "duplicate pod uid"};
    if (i == rerr.at) rerr.rethrow();
    const uint32_t s = spec_of[i];
    if (spec_rep[s] != i) continue;
    if (s == aerr.at) aerr.rethrow();
    pod_phase_b(i, work[s]);
  }
  // <U> Topology.Update after a relaxation: every spread keyed under the
  // relaxed filter joins the group of that hash; a hash no pod's first
  // variant keys is a group created at that moment (lazy), in spec order
  for (uint32_t s = 0; s < NS; s++) pod_phase_b2(s, work[s]);
  par_try(NS, 8, [&](uint32_t s) { pod_phase_c(work[s]); }).rethrow();
  spec_aff_text.assign(NS, std::string());
  spec_pref_keys.assign(NS, {});
  for (uint32_t s = 0; s < NS; s++) {
    spec_aff_text[s] = std::move(work[s].aff_text);
    spec_pref_keys[s] = std::move(work[s].pref_keys);
  }
  return work;
}

// spec variants (e.variants), then the device variants: each pod's
// spec's variants in order (e.var_sv: device variant -> spec variant)
void Ctx::pod_variants(std::vector<PodWork> work) {
  const uint32_t NS = (uint32_t)spec_rep.size();
  sv_begin.assign(NS, 0);
  sv_count.assign(NS, 0);
  std::vector<std::vector<uint32_t>> spec_var_state(NS);
  for (uint32_t s = 0; s < NS; s++) {
    spec_var_state[s] = std::move(work[s].var_state);
    sv_begin[s] = (uint32_t)e.variants.size();
    sv_count[s] = (uint32_t)work[s].vars.size();
    for (auto& v : work[s].vars) e.variants.push_back(std::move(v));
    for (auto& t : work[s].var_tols) variant_tols.push_back(std::move(t));
  }
  // a group's first owner variant: the first variant of its first owner
  // spec (lazy groups: the first in the state that keys them)
  for (auto& g : groups) {
    if (g.owner_spec == gsd::NONE) continue;
    g.owner_sv = sv_begin[g.owner_spec];
    if (!g.lazy) continue;
    const auto& vs = spec_var_state[g.owner_spec];
    uint32_t k = 0;
    while (k < vs.size() && vs[k] != g.owner_state) k++;
    if (k == vs.size()) throw Fail{GS_E_INVALID, "internal: lazy topology group without its relaxation state"};
    g.owner_sv += k;
  }
  e.var_begin.resize(e.P);
  e.var_count.resize(e.P);
  uint32_t nv = 0;
  for (uint32_t i = 0; i < e.P; i++) {
    e.var_begin[i] = nv;
    e.var_count[i] = sv_count[spec_of[i]];
    nv += e.var_count[i];
  }
  e.var_sv.resize(nv);
  par_for(e.P, 2048, [&](uint32_t i) {
    const uint32_t b = sv_begin[spec_of[i]];
    for (uint32_t k = 0; k < e.var_count[i]; k++) e.var_sv[e.var_begin[i] + k] = b + k;
  });
  e.V = nv;
}

// device variant records; identical has-bitsets share one arena slot and
// identical IT-key requirement sets one class
void Ctx::pod_var_records() {
  e.vars.resize(e.V);
  e.var_itclass.assign(e.V, gsd::NONE);
  std::map<std::vector<uint64_t>, uint32_t> arena_slot, itclass_of;
  std::vector<std::vector<uint32_t>> class_offs;  // per class: arena offset per IT key (NONE: unconstrained)
  auto arena = [&](const std::vector<uint64_t>& words) {
    auto f = arena_slot.find(words);
    if (f != arena_slot.end()) return f->second;
    const uint32_t off = (uint32_t)e.itmask.size();
    e.itmask.insert(e.itmask.end(), words.begin(), words.end());
    arena_slot.emplace(words, off);
    return off;
  };
  // one record per spec variant (serial: arena slots, classes and free-key
  // entries in first-use order), then every device variant a copy of its
  // spec variant's with its pod and index
  const uint32_t SV = (uint32_t)e.variants.size();
  std::vector<gsd::VarRec> sv_rec(SV);
  std::vector<uint32_t> sv_itclass(SV, gsd::NONE);
  for (uint32_t sv = 0; sv < SV; sv++) {
    auto& pv = e.variants[sv];
    gsd::VarRec& vr = sv_rec[sv];
    std::memset(&vr, 0, sizeof vr);
    for (int k = 0; k < gsd::KMAX_IT; k++) vr.itmask_off[k] = gsd::NONE;
    bool itk = false;
    for (uint32_t k = 0; k < e.K; k++) {
      auto f = pv.reqs.find(e.it_keys[k]);
      if (f == pv.reqs.end()) continue;
      vr.itmask_off[k] = arena(f->second.has.w);
      itk = true;
    }
    if (itk) {
      // the class key: the arena slots of the constrained keys
      std::vector<uint64_t> sig(vr.itmask_off, vr.itmask_off + e.K);
      auto f = itclass_of.find(sig);
      if (f == itclass_of.end()) {
        f = itclass_of.emplace(sig, (uint32_t)class_offs.size()).first;
        class_offs.emplace_back(vr.itmask_off, vr.itmask_off + e.K);
      }
      sv_itclass[sv] = f->second;
    }
    vr.zfull_off = vr.cfull_off = gsd::NONE;
    for (int kk = 0; kk < 2; kk++) {
      auto f = pv.reqs.find(kk ? e.k_ct : e.k_zone);
      if (f == pv.reqs.end()) continue;
      (kk ? vr.cfull_off : vr.zfull_off) = arena(f->second.has.w);
    }
    vr.zm = zone_has(pv.reqs);
    vr.cm = ct_has(pv.reqs);
    vr.ctb = ct_bits(pv.reqs) | (pv.reqs.empty() && pv.own.empty() ? gsd::VF_SIMPLE : 0u);
    // owns a zone spread group: only those read the per-pod minimum counts
    for (uint32_t g : pv.own)
      if (groups[g].sp.key != kHostname && groups[g].kind == 0) vr.ctb |= gsd::VF_ZSPREAD;
    // hostname-only topology (spread, anti-affinity, inverse, host ports;
    // not pod affinity): the wave kernel's fast accept reads the counts
    if (pv.reqs.empty() && !pv.own.empty() && pv.own.size() <= 4) {
      bool host = true;
      for (uint32_t g : pv.own) host = host && groups[g].sp.key == kHostname && groups[g].kind != 4;
      if (host) vr.ctb |= gsd::VF_HOSTFA;
    }
    vr.zs = zone_full(pv.strict);
    vr.zn = zone_full(pv.reqs);
    vr.zflags = zone_flags(pv.reqs);
    vr.tol = vr.tolt = 0;  // build_taint_classes
    vr.fk_begin = (uint32_t)e.fk_entries.size();
    for (auto& kv : pv.reqs) {
      const Key& key = e.keys[kv.first];
      if (key.cls != KEY_FREE && key.shadow < 0) continue;
      gsd::FKEntry fe{};
      fe.slot = (uint32_t)(key.cls == KEY_FREE ? key.slot : key.shadow);
      fe.st = to_fk(kv.second);
      e.fk_entries.push_back(fe);
      // the existing-node check of a shadowed key runs on its free slot
      // (the IT-key class above already has this key's mask)
      if (key.cls == KEY_IT) vr.itmask_off[key.slot] = gsd::NONE;
      else if (key.cls == KEY_ZONE) vr.zfull_off = gsd::NONE;
      else vr.cfull_off = gsd::NONE;
    }
    vr.fk_count = (uint32_t)e.fk_entries.size() - vr.fk_begin;

  }
  par_for(e.P, 1024, [&](uint32_t i) {
    for (uint32_t v = e.var_begin[i]; v < e.var_begin[i] + e.var_count[i]; v++) {
      e.vars[v] = sv_rec[e.var_sv[v]];
      e.vars[v].pod = i;
      e.vars[v].vix = v;
      e.var_itclass[v] = sv_itclass[e.var_sv[v]];
    }
  });
  if (e.itmask.empty()) e.itmask.push_back(0);
  e.itclass_mask.assign(std::max<size_t>(class_offs.size(), 1) * e.W, 0);
  for (size_t c = 0; c < class_offs.size(); c++)
    for (uint32_t it = 0; it < e.N; it++) {
      bool ok = true;
      for (uint32_t k = 0; k < e.K && ok; k++) {
        const uint32_t off = class_offs[c][k];
        if (off == gsd::NONE) continue;
        const uint32_t vid = e.it_vid[(size_t)k * e.N + it];
        ok = (e.itmask[off + (vid >> 6)] >> (vid & 63)) & 1;
      }
      if (ok) e.itclass_mask[c * e.W + it / 64] |= 1ull << (it % 64);
    }
  if (e.fk_entries.empty()) e.fk_entries.push_back(gsd::FKEntry{});
}

// <U> NewQueue: cpu desc, memory desc, creationTimestamp asc, UID asc (total order)
// sorted on packed keys: the UID's first 8 bytes (big-endian, so integer
// order is byte order) decide most ties without touching the strings
// the fields as order-preserving unsigned integers (cpu and memory
// descending, creation time ascending; signed -> unsigned by flipping the
// sign bit) and the UID's first 8 bytes, in two 128-bit words: the sort
// compares integers; keys that tie (UIDs sharing 8 bytes) are put in full
// order afterwards
void Ctx::pod_queue_order() {
  std::vector<int64_t> cpu(e.P, 0), mem(e.P, 0);
  auto rc = rid_map.find("cpu"), rmm = rid_map.find("memory");
  for (uint32_t i = 0; i < e.P; i++) {
    if (rc != rid_map.end()) cpu[i] = e.pod_req[(size_t)i * e.R + rc->second];
    if (rmm != rid_map.end()) mem[i] = e.pod_req[(size_t)i * e.R + rmm->second];
  }
  struct QK {
    unsigned __int128 k, k2;
    uint32_t i;
  };
  std::vector<QK> qk(e.P);
  par_for(e.P, 4096, [&](uint32_t i) {
    const std::string& u = strs[p->pods[i].uid];  // checked by the uid pass
    uint64_t x = 0;
    for (size_t b = 0; b < 8; b++) x = (x << 8) | (b < u.size() ? (uint8_t)u[b] : 0u);
    auto bias = [](int64_t v) { return (uint64_t)v ^ (1ull << 63); };
    qk[i] = QK{((unsigned __int128)~bias(cpu[i]) << 64) | ~bias(mem[i]),
               ((unsigned __int128)bias(p->pods[i].creation_ns) << 64) | x, i};
  });
  tm.sub("queue_keys");
  auto kless = [](const QK& a, const QK& b) { return a.k != b.k ? a.k < b.k : a.k2 < b.k2; };
  auto qless = [&](const QK& a, const QK& b) {
    if (a.k != b.k) return a.k < b.k;
    if (a.k2 != b.k2) return a.k2 < b.k2;
    return strs[p->pods[a.i].uid] < strs[p->pods[b.i].uid];
  };
  // a total order (uids are unique): the result is the one order whatever the
  // sort's split
  par_sort(qk, kless);
  // runs of equal keys (UIDs that share their first 8 bytes): full order
  for (uint32_t a = 0; a < e.P;) {
    uint32_t b = a + 1;
    while (b < e.P && qk[b].k == qk[a].k && qk[b].k2 == qk[a].k2) b++;
    if (b - a > 1) std::sort(qk.begin() + a, qk.begin() + b, qless);
    a = b;
  }
  e.queue0.resize(e.P);
  for (uint32_t k = 0; k < e.P; k++) e.queue0[k] = qk[k].i;
}

}  // namespace gsh::enc
