// encode_topology.cpp — the encoder's topology and volume phases: a pod's
// spreads, (anti-)affinity terms and host ports as encoder types, the topology
// groups' device records, counts and lists, and the CSI volume limits.
#include "encode_ctx.hpp"

#include <arpa/inet.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <numeric>

namespace gsh::enc {

std::map<std::string, std::string> Ctx::label_map(gs_range r) const {
  chk(r, p->n_labels, "labels");
  std::map<std::string, std::string> m;
  for (uint32_t i = 0; i < r.count; i++) m[S(p->labels[r.begin + i].key)] = S(p->labels[r.begin + i].value);
  return m;
}
std::vector<SpreadEnc> Ctx::spreads_of(const gs_pod& pd) const {
  chk(pd.spreads, p->n_spreads, "spreads");
  std::vector<SpreadEnc> out;
  for (uint32_t k = 0; k < pd.spreads.count; k++) {
    const gs_spread& q = p->spreads[pd.spreads.begin + k];
    SpreadEnc sp;
    sp.key = label_normalize(S(q.topology_key));
    if (sp.key != kZone && sp.key != kHostname && sp.key != kCapacityType && sp.key != kNodePool)
      throw Fail{GS_E_UNSUPPORTED, "topology spread key other than zone / capacity type / NodePool / hostname"};
    if (sp.key != kHostname && sp.key != e.keys[e.k_dom].name)
      throw Fail{GS_E_UNSUPPORTED, "topology spreads on more than one of the zone, capacity-type and NodePool keys"};
    if (q.max_skew < 1) throw Fail{GS_E_INVALID, "maxSkew < 1"};
    if (q.when_unsatisfiable > GS_SPREAD_SCHEDULE_ANYWAY || q.node_affinity_policy > GS_POLICY_IGNORE ||
        q.node_taints_policy > GS_POLICY_IGNORE)
      throw Fail{GS_E_INVALID, "bad topology spread enum"};
    // nodeTaintsPolicy Honor (TopologyNodeFilter.Matches: the owner's
    // tolerations must tolerate a node's / NodeClaim's taints for it to
    // count and for its domain to enter the minimum) is accepted when the
    // owner tolerates every taint of the problem, where it equals Ignore;
    // checked in build_nodes once every taint is known
    sp.honor_taints = q.node_taints_policy == GS_POLICY_HONOR;
    sp.skew = q.max_skew;
    sp.mind = q.min_domains > 0 ? q.min_domains : 0;
    sp.sa = q.when_unsatisfiable == GS_SPREAD_SCHEDULE_ANYWAY;
    sp.has_sel = q.has_selector != 0;
    sp.ignore_aff = q.node_affinity_policy == GS_POLICY_IGNORE;
    sp.ml = label_map(q.match_labels);
    chk(q.match_expressions, p->n_reqs, "reqs");
    for (uint32_t x = 0; x < q.match_expressions.count; x++) {
      const gs_requirement& r = p->reqs[q.match_expressions.begin + x];
      if (r.op > GS_OP_DOES_NOT_EXIST) throw Fail{GS_E_INVALID, "label selector operator"};
      chk(r.values, p->n_value_ids, "values");
      std::set<std::string> vals;
      for (uint32_t v = 0; v < r.values.count; v++) vals.insert(S(p->value_ids[r.values.begin + v]));
      sp.ex.emplace_back(S(r.key), r.op, std::move(vals));
    }
    // matchLabelKeys: key In [the pod's value] for every key the pod carries
    chk(q.match_label_keys, p->n_value_ids, "values");
    if (q.match_label_keys.count) {
      const auto labels = label_map(pd.labels);
      for (uint32_t m = 0; m < q.match_label_keys.count; m++) {
        const std::string& k = S(p->value_ids[q.match_label_keys.begin + m]);
        auto f = labels.find(k);
        if (f != labels.end()) sp.ex.emplace_back(k, (uint32_t)GS_OP_IN, std::set<std::string>{f->second});
      }
    }
    out.push_back(std::move(sp));
  }
  return out;
}
std::vector<AntiEnc> Ctx::antis_of(const gs_pod& pd) const { return terms_of(pd, pd.anti_affinity, false); }
// zone-key anti-affinity is deterministic (every empty zone both sides
// allow); zone-key pod affinity bootstraps on a zone picked in Go map order
std::vector<AntiEnc> Ctx::terms_of(const gs_pod& pd, gs_range rg, bool affinity) const {
  chk(rg, p->n_affinity_terms, "affinity_terms");
  std::vector<AntiEnc> out;
  for (uint32_t k = 0; k < rg.count; k++) {
    const gs_affinity_term& q = p->affinity_terms[rg.begin + k];
    const std::string tk = label_normalize(S(q.topology_key));
    if (tk != kHostname && !(tk == kZone && !affinity))
      throw Fail{GS_E_UNSUPPORTED, affinity ? "pod affinity topologyKey other than hostname"
                                            : "pod anti-affinity topologyKey other than hostname / zone"};
    if (e.k_dom != e.k_zone && tk == kZone)
      throw Fail{GS_E_UNSUPPORTED, "zone-key pod anti-affinity beside capacity-type / NodePool topology spreads"};
    AntiEnc a;
    a.required = q.required != 0;
    a.weight = q.weight;
    a.sel.key = tk;
    a.sel.has_sel = q.has_selector != 0;
    a.sel.ml = label_map(q.match_labels);
    chk(q.match_expressions, p->n_reqs, "reqs");
    for (uint32_t x = 0; x < q.match_expressions.count; x++) {
      const gs_requirement& r = p->reqs[q.match_expressions.begin + x];
      if (r.op > GS_OP_DOES_NOT_EXIST) throw Fail{GS_E_INVALID, "label selector operator"};
      chk(r.values, p->n_value_ids, "values");
      std::set<std::string> vals;
      for (uint32_t v = 0; v < r.values.count; v++) vals.insert(S(p->value_ids[r.values.begin + v]));
      a.sel.ex.emplace_back(S(r.key), r.op, std::move(vals));
    }
    // <U> buildNamespaceList: the listed namespaces plus those the
    // namespaceSelector matches; neither = the pod's namespace
    chk(q.namespaces, p->n_value_ids, "values");
    for (uint32_t v = 0; v < q.namespaces.count; v++) a.nss.insert(S(p->value_ids[q.namespaces.begin + v]));
    if (q.has_ns_selector) {
      SpreadEnc nsel;
      nsel.has_sel = true;
      nsel.ml = label_map(q.ns_match_labels);
      chk(q.ns_match_expressions, p->n_reqs, "reqs");
      for (uint32_t x = 0; x < q.ns_match_expressions.count; x++) {
        const gs_requirement& r = p->reqs[q.ns_match_expressions.begin + x];
        if (r.op > GS_OP_DOES_NOT_EXIST) throw Fail{GS_E_INVALID, "label selector operator"};
        chk(r.values, p->n_value_ids, "values");
        std::set<std::string> vals;
        for (uint32_t v = 0; v < r.values.count; v++) vals.insert(S(p->value_ids[r.values.begin + v]));
        nsel.ex.emplace_back(S(r.key), r.op, std::move(vals));
      }
      chk(gs_range{0, p->n_namespaces}, p->n_namespaces, "namespaces");
      for (uint32_t n = 0; n < p->n_namespaces; n++)
        if (nsel.matches(label_map(p->namespaces[n].labels))) a.nss.insert(S(p->namespaces[n].name));
    } else if (a.nss.empty()) {
      a.nss.insert(S(pd.ns));
    }
    out.push_back(std::move(a));
  }
  return out;
}
std::vector<PortEnc> Ctx::ports_of(const gs_pod& pd) const {
  chk(pd.host_ports, p->n_host_ports, "host_ports");
  std::vector<PortEnc> out;
  static const std::array<uint8_t, 16> z6{}, z4{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff, 0, 0, 0, 0};
  for (uint32_t k = 0; k < pd.host_ports.count; k++) {
    const gs_host_port& q = p->host_ports[pd.host_ports.begin + k];
    if (q.port < 1 || q.port > 65535) throw Fail{GS_E_INVALID, "host port out of range"};
    PortEnc e;
    e.proto = S(q.protocol).empty() ? std::string("TCP") : S(q.protocol);
    e.port = q.port;
    const std::string& ip = S(q.ip);
    in_addr b4;
    std::array<uint8_t, 16> b6;
    e.ip = z4;  // unparsable: 0.0.0.0
    if (inet_pton(AF_INET, ip.c_str(), &b4) == 1) std::memcpy(e.ip.data() + 12, &b4, 4);
    else if (inet_pton(AF_INET6, ip.c_str(), b6.data()) == 1) e.ip = b6;
    e.unspec = e.ip == z6 || e.ip == z4;
    out.push_back(e);
  }
  return out;
}
PodSel Ctx::sel_of(const gs_pod& pd) const {
  PodSel ps;
  ps.ns = S(pd.ns);
  ps.labels = label_map(pd.labels);
  for (auto& a : antis_of(pd))
    if (a.required) ps.carried.insert(a.hash());
  ps.ports = ports_of(pd);
  return ps;
}
bool Ctx::group_counts(const GroupEnc& g, const PodSel& ps) const {
  switch (g.kind) {
    case 0: return ps.ns == g.ns && g.sp.matches(ps.labels);
    case 1:
    case 4: return g.anti.selects(ps.ns, ps.labels);
    case 2: return ps.carried.count(g.inv_hash) != 0;
    default:
      for (auto& e : ps.ports)
        if (e.matches(g.port)) return true;
      return false;
  }
}
uint32_t Ctx::group_id(const std::string& h, GroupEnc&& g) {
  auto f = group_idx.find(h);
  if (f == group_idx.end()) {
    if (groups.size() >= (size_t)gsd::TGMAX) throw Fail{GS_E_UNSUPPORTED, "more than 4096 topology groups"};
    f = group_idx.emplace(h, (uint32_t)groups.size()).first;
    groups.push_back(std::move(g));
  }
  return f->second;
}
// a group admitting an owner only where the count is 0: on the hostname key
// through count + self <= skew = self; on the zone key (anti-affinity and
// its inverse) the domains with count 0 (TK_ANTI)
GroupEnc Ctx::host_group(int kind, bool self, const std::string& key) const {
  GroupEnc g;
  g.kind = kind;
  g.sp.key = key;
  g.sp.skew = self ? 1 : 0;
  return g;
}

// <U> VolumeUsage (ExistingNode.CanAdd's ExceedsLimits): per node the
// distinct volumes of its bound pods per driver and the CSINode limits; a
// node already over a limit takes no pod at all (the union check fails
// whatever the pod mounts)
// A volume only one pod mounts (pods and bound pods, a bound pod that is
// also in the pod list -- consolidation -- counting once) can never be on a
// node the pod is placed on: it is a per-driver count of "fresh" volumes.
// The others (<= 64 distinct) are bits a node may already hold.
void Ctx::build_volumes() {
  std::map<std::string, uint32_t> drv;
  std::map<std::pair<std::string, std::string>, uint32_t> vol;
  std::map<std::pair<std::string, std::string>, std::set<uint32_t>> users;
  auto volkey = [&](const gs_volume& v) { return std::make_pair(S(v.driver), S(v.id)); };
  for (uint32_t i = 0; i < e.P; i++) {
    const gs_pod& pd = p->pods[i];
    chk(pd.volumes, p->n_volumes, "volumes");
    for (uint32_t k = 0; k < pd.volumes.count; k++) users[volkey(p->volumes[pd.volumes.begin + k])].insert(i);
  }
  if (p->n_bound_pods && !p->bound_pod_node) throw Fail{GS_E_INVALID, "bound pods without their nodes"};
  for (uint32_t b = 0; b < p->n_bound_pods; b++) {
    const gs_pod& bp = p->bound_pods[b];
    chk(bp.volumes, p->n_volumes, "volumes");
    const uint32_t who = bound_alias != gsd::NONE ? bound_alias + b : e.P + b;
    for (uint32_t k = 0; k < bp.volumes.count; k++) {
      auto f = users.find(volkey(p->volumes[bp.volumes.begin + k]));
      if (f != users.end()) f->second.insert(who);  // only volumes pods in the list mount matter
    }
  }
  // without pending volumes the kernels never read these (any_vol)
  const size_t PV = users.empty() ? 1 : std::max<uint32_t>(e.P, 1);
  e.pod_vol.assign(PV * gsd::VDMAX, 0);
  e.pod_vfresh.assign(PV * gsd::VDMAX, 0);
  for (uint32_t i = 0; i < e.P; i++) {
    const gs_pod& pd = p->pods[i];
    if (!pd.volumes.count) continue;
    std::set<std::pair<std::string, std::string>> mine;
    for (uint32_t k = 0; k < pd.volumes.count; k++) mine.insert(volkey(p->volumes[pd.volumes.begin + k]));
    for (auto& vk : mine) {
      const uint32_t d = drv.emplace(vk.first, (uint32_t)drv.size()).first->second;
      if (d >= (uint32_t)gsd::VDMAX) throw Fail{GS_E_UNSUPPORTED, "pending pods mount volumes of more than 4 CSI drivers"};
      if (users[vk].size() < 2) {
        e.pod_vfresh[(size_t)i * gsd::VDMAX + d]++;
        continue;
      }
      const uint32_t b = vol.emplace(vk, (uint32_t)vol.size()).first->second;
      if (b >= 64) throw Fail{GS_E_UNSUPPORTED, "pods share more than 64 distinct volumes"};
      e.pod_vol[(size_t)i * gsd::VDMAX + d] |= 1ull << b;
    }
  }
  std::vector<uint32_t> pos_of(e.NN);
  for (uint32_t i = 0; i < e.NN; i++) pos_of[e.node_order[i]] = i;
  std::vector<std::map<std::string, std::set<std::string>>> used(e.NN);
  if (p->n_bound_pods && !p->bound_pod_node) throw Fail{GS_E_INVALID, "bound pods without their nodes"};
  for (uint32_t b = 0; b < p->n_bound_pods; b++) {
    const gs_pod& bp = p->bound_pods[b];
    if (p->bound_pod_node[b] >= e.NN) throw Fail{GS_E_INVALID, "bound pod node out of range"};
    chk(bp.volumes, p->n_volumes, "volumes");
    for (uint32_t k = 0; k < bp.volumes.count; k++) {
      const gs_volume& v = p->volumes[bp.volumes.begin + k];
      used[pos_of[p->bound_pod_node[b]]][S(v.driver)].insert(S(v.id));
    }
  }
  e.n_vol.assign(std::max<uint32_t>(e.NN, 1), gsd::NodeVol{});
  for (uint32_t pos = 0; pos < e.NN; pos++) {
    const gs_node& g = p->nodes[e.node_order[pos]];
    chk(g.volume_limits, p->n_volume_limits, "volume_limits");
    std::map<std::string, int64_t> lim;
    for (uint32_t k = 0; k < g.volume_limits.count; k++)
      lim[S(p->volume_limits[g.volume_limits.begin + k].driver)] = p->volume_limits[g.volume_limits.begin + k].limit;
    gsd::NodeVol& nv = e.n_vol[pos];
    for (int d = 0; d < gsd::VDMAX; d++) nv.lim[d] = INT32_MAX;
    for (auto& kv : used[pos]) {
      auto f = lim.find(kv.first);
      if (f != lim.end() && (int64_t)kv.second.size() > f->second) e.nodes[pos].ok = 0;  // already over
    }
    for (auto& dv : drv) {
      auto f = lim.find(dv.first);
      if (f != lim.end()) nv.lim[dv.second] = (int32_t)std::max<int64_t>(f->second, -1);
      auto u = used[pos].find(dv.first);
      nv.cnt[dv.second] = u == used[pos].end() ? 0 : (int32_t)u->second.size();
    }
    for (auto& vv : vol) {
      auto u = used[pos].find(vv.first.first);
      if (u != used[pos].end() && u->second.count(vv.first.second)) nv.present |= 1ull << vv.second;
    }
  }
  e.any_vol = !drv.empty() && e.NN > 0;
}

// the domain universe (In values of NodePool requirements of NodePools that
// have instance types, existing nodes' labels) and every group's device record
void Ctx::topo_group_records() {
  const Vocab& zv = e.keys[e.k_dom].vocab;
  bool any_zone = false;
  for (auto& g : groups) any_zone = any_zone || g.sp.key != kHostname;
  if (any_zone && zv.size() > (size_t)gsd::ZVMAX)
    throw Fail{GS_E_UNSUPPORTED, "zone / capacity-type topology groups over more than 63 domain values"};
  e.NZV = (uint32_t)std::min<size_t>(zv.size() - 1, gsd::ZVMAX);
  e.ZS = std::max<uint32_t>(e.NZV, 1);
  e.zone_order.resize(e.NZV);
  std::iota(e.zone_order.begin(), e.zone_order.end(), 0);
  std::sort(e.zone_order.begin(), e.zone_order.end(), [&](uint32_t a, uint32_t b) { return zv.vals[a] < zv.vals[b]; });
  e.zone_cat.assign(gsd::ZVMAX, gsd::NONE);
  if (e.dom_np) {
    // a NodePool domain narrows no catalog zone or capacity type
  } else if (e.dom_ct) {
    for (uint32_t c = 0; c < e.C; c++)
      if (e.cat_ct[c] < (uint32_t)gsd::ZVMAX) e.zone_cat[e.cat_ct[c]] = c;
  } else {
    for (uint32_t z = 0; z < e.Z; z++)
      if (e.cat_zone[z] < (uint32_t)gsd::ZVMAX) e.zone_cat[e.cat_zone[z]] = z;
  }
  // <U> buildDomainGroups inserts Requirement.Values() of each NodePool's
  // requirements combined with each of its instance types': for a NotIn
  // those are the excluded values (this restatement takes In values only),
  // and an instance type's own requirement on the key would add its values.
  // The IBM catalog's instance types carry neither a zone nor a capacity
  // type (instancetype.go:719-724), so an unconstrained NodePool provides
  // no domain either way; the two ambiguous forms are refused, not guessed
  if (any_zone) {
    for (auto& u : np_universe) {
      if (!u.second) continue;
      auto f = u.first.find(e.k_dom);
      if (f != u.first.end() && f->second.comp && !f->second.excl.none())
        throw Fail{GS_E_UNSUPPORTED, "a NodePool NotIn requirement on the topology spread key " + e.keys[e.k_dom].name};
    }
    for (uint32_t k : e.it_keys)
      if (k == e.k_dom)
        throw Fail{GS_E_UNSUPPORTED, "instance types with a requirement on the topology spread key " + e.keys[e.k_dom].name};
  }
  uint64_t known_zone = 0;
  for (auto& u : np_universe) {
    if (!u.second) continue;
    auto f = u.first.find(e.k_dom);
    if (f != u.first.end() && !f->second.comp) known_zone |= f->second.has.w[0];  // operator In
  }
  e.known_np = known_zone;
  e.zone_nodes.assign(gsd::ZVMAX, 0);
  for (auto& nr : e.nodes)
    if (nr.dvid < e.ZS) {
      known_zone |= 1ull << nr.dvid;
      e.zone_nodes[nr.dvid]++;
    }
  e.zknown0 = known_zone;
  e.tgroups.assign(e.TG, gsd::TGroupRec{});
  for (uint32_t g = 0; g < e.TG; g++) {
    gsd::TGroupRec& t = e.tgroups[g];
    t.skew = groups[g].sp.skew;
    // a lazy group's minDomains is its creator's, known at the Relax that
    // creates it: -(lazy index + 1) reads the kernels' lazy minDomains
    t.mind = groups[g].lazy ? -(int32_t)groups[g].lazy_idx - 1 : groups[g].sp.mind;
    const int kind = groups[g].kind;
    if (groups[g].sp.key == kHostname) {
      t.kind = gsd::TK_HOST | (kind == 4 ? gsd::TK_AFF : 0u);
      t.slot = e.TGH++;
    } else {
      t.kind = kind == 1 || kind == 2 ? gsd::TK_ANTI : 0u;
      t.slot = e.TGZ++;
      t.known0 = known_zone;
    }
  }
}

// <U> TopologyDomainGroup.ForEachDomain under TaintPolicy Honor: a domain
// enters domainMinCount only if a NodePool (with instance types) or a node
// providing it has taints the pod (this relaxation) tolerates.  Folded into
// the variant's strict domains, which only the minimum reads (topo_tmin)
void Ctx::topo_honor_domains() {
  bool any_honor = false;
  for (auto& g : groups) any_honor = any_honor || (g.kind == 0 && g.sp.honor_taints && g.sp.key != kHostname);
  if (any_honor) {
    std::vector<std::pair<uint64_t, uint64_t>> prov;  // (taint classes, domains)
    for (size_t i = 0; i < np_universe.size(); i++) {
      if (!np_universe[i].second) continue;
      auto f = np_universe[i].first.find(e.k_dom);
      if (f == np_universe[i].first.end() || f->second.comp) continue;
      uint64_t cm = 0;
      for (uint32_t id : np_universe_taints[i]) cm |= 1ull << taint_cls[id];
      prov.emplace_back(cm, f->second.has.w[0]);
    }
    for (auto& nr : e.nodes)
      if (nr.dvid < e.ZS) prov.emplace_back(nr.taints, 1ull << nr.dvid);
    for (uint32_t v = 0; v < e.V; v++) {
      const uint32_t sv = e.var_sv[v];
      uint32_t nh = 0, ni = 0;
      for (uint32_t g : e.variants[sv].own)
        if (groups[g].kind == 0 && groups[g].sp.key != kHostname) (groups[g].sp.honor_taints ? nh : ni)++;
      if (!nh) continue;
      if (ni)
        throw Fail{GS_E_UNSUPPORTED, "a pod owning zone-key spreads with both nodeTaintsPolicy Honor and Ignore"};
      // a domain no NodePool or node provides (one a Record adds during
      // the Solve) has no taints to tolerate: it stays
      uint64_t dm = 0, provided = 0;
      for (auto& pr : prov) {
        provided |= pr.second;
        if ((pr.first & ~final_sv_tol[sv]) == 0) dm |= pr.second;
      }
      e.vars[v].zs &= dm | ~provided;
    }
  }
}

// the counts of the selected bound pods, per domain and per node
void Ctx::topo_count_bound(const SelIndex& six) {
  std::vector<uint32_t> pos_of(e.NN);
  for (uint32_t i = 0; i < e.NN; i++) pos_of[e.node_order[i]] = i;
  if (p->n_bound_pods && !p->bound_pod_node) throw Fail{GS_E_INVALID, "bound pods without their nodes"};
  std::vector<uint32_t> cand;
  // <U> countDomains under AffinityPolicy Honor: a bound pod counts only on
  // a node whose labels (+ hostname) are strictly Compatible with one of the
  // group's filter terms (oracle/solve.cpp TGroup::filter_matches)
  std::vector<std::unique_ptr<Reqs>> nreqs(e.NN);
  auto node_matches = [&](const SpreadEnc& sp, uint32_t raw) {
    if (!nreqs[raw]) {
      const gs_node& g = p->nodes[raw];
      nreqs[raw].reset(new Reqs(node_labels_reqs(g.labels)));
      reqs_add(e, *nreqs[raw], e.k_hostname, in_one_or_omega(e.k_hostname, S(g.name)));
    }
    for (auto& f : sp.filter)
      if (reqs_compatible(e, *nreqs[raw], f, false)) return true;
    return false;
  };
  // nodeTaintsPolicy Honor: the group's first owner's tolerations (before
  // Relax) against a bound pod's Node taints in countDomains
  auto node_tolerated = [&](uint32_t g, uint32_t raw) {
    const std::vector<Tol>& tols = variant_tols[groups[g].owner_sv];
    const gs_range r = p->nodes[raw].taints;
    chk(r, p->n_taints, "taints");
    for (uint32_t k = 0; k < r.count; k++) {
      const gs_taint& t = p->taints[r.begin + k];
      if (!tolerated(tols, TaintKey{S(t.key), S(t.value), S(t.effect)})) return false;
    }
    return true;
  };
  for (uint32_t b = 0; b < p->n_bound_pods; b++) {
    const gs_pod& bp = p->bound_pods[b];
    if (p->bound_pod_node[b] >= e.NN) throw Fail{GS_E_INVALID, "bound pod node out of range"};
    const uint32_t pos = pos_of[p->bound_pod_node[b]];
    const PodSel ps = sel_of(bp);
    six.candidates(ps, &cand);
    for (uint32_t g : cand) {
      if (!group_counts(groups[g], ps)) continue;
      if (groups[g].kind == 0 && groups[g].sp.strict_aff && !node_matches(groups[g].sp, p->bound_pod_node[b]))
        continue;
      if (groups[g].kind == 0 && groups[g].sp.honor_taints && !node_tolerated(g, p->bound_pod_node[b])) continue;
      gsd::TGroupRec& t = e.tgroups[g];
      if (t.kind & gsd::TK_HOST) {
        e.hn0[(size_t)t.slot * e.NN + pos]++;
        e.htot0[t.slot]++;  // the total over domains (affinity bootstrap)
      } else {
        const uint32_t z = e.nodes[pos].dvid;
        if (z == gsd::NONE || z >= e.ZS) continue;
        e.zcnt0[(size_t)t.slot * e.ZS + z]++;
        e.zn_cnt[(size_t)t.slot * e.NN + pos]++;
        t.known0 |= 1ull << z;
      }
    }
  }
}

// per spec: the selection list (shared by its pods' variants), then each
// spec variant's own list with the self flag; a pod's variants point at
// its spec's lists
void Ctx::topo_lists(const SelIndex& six) {
  std::vector<uint32_t> cand;
  // nodeTaintsPolicy Honor: the group's first owner's tolerated taint classes
  // for the counted specs
  std::vector<uint64_t> g_otol(e.TG, ~0ull);
  for (uint32_t g = 0; g < e.TG; g++)
    if (groups[g].kind == 0 && groups[g].sp.honor_taints) g_otol[g] = final_sv_tol[groups[g].owner_sv];
  e.tg_list.clear();
  std::vector<uint8_t> selected(e.TG, 0);
  std::vector<uint32_t> mine;
  const uint32_t NS = (uint32_t)spec_rep.size();
  std::vector<uint32_t> sel_off(NS), sel_n(NS), own_off(e.variants.size()), own_n(e.variants.size());
  for (uint32_t s = 0; s < NS; s++) {
    six.candidates(pod_sel[s], &cand);
    mine.clear();
    for (uint32_t g : cand)
      if (group_counts(groups[g], pod_sel[s])) mine.push_back(g);
    for (uint32_t g : mine) {
      // taint Honor: every NodeClaim / node a counted pod can land on (it
      // tolerates the taints) must be one the owner tolerates, in every
      // relaxation of the pod (Relax may add the PreferNoSchedule toleration)
      if (groups[g].kind == 0 && groups[g].sp.honor_taints)
        for (uint32_t sv = sv_begin[s]; sv < sv_begin[s] + sv_count[s]; sv++)
          if (final_sv_tol[sv] & ~g_otol[g])
            throw Fail{GS_E_UNSUPPORTED, "a pod counted by a topology spread (nodeTaintsPolicy Honor) tolerating a "
                                         "taint its owner does not"};
    }
    for (uint32_t g : mine) {
      const SpreadEnc& sp = groups[g].sp;
      if (groups[g].kind != 0 || !sp.strict_aff) continue;
      // the NodeClaims / nodes this spec lands on match the owner's filter
      // only if it carries the same terms and no preference narrows them
      if (spec_aff_text[s] != sp.ftext)
        throw Fail{GS_E_UNSUPPORTED,
                   "a pod counted by a topology spread (nodeAffinityPolicy Honor) without its owner's node affinity"};
      for (uint32_t k : spec_pref_keys[s])
        for (auto& f : sp.filter)
          if (f.count(k))
            throw Fail{GS_E_UNSUPPORTED,
                       "a pod counted by a topology spread (nodeAffinityPolicy Honor) with preferred node affinity "
                       "on a key of the spread's filter"};
    }
    sel_off[s] = (uint32_t)e.tg_list.size();
    sel_n[s] = (uint32_t)mine.size();
    for (uint32_t g : mine) {
      selected[g] = 1;
      if (groups[g].lazy)  // slots and lazy indices < 4096: slot in bits 0..11, lazy index in 12..23
        e.tg_list.push_back(e.tgroups[g].slot | (groups[g].lazy_idx << 12) | ((e.tgroups[g].kind | gsd::TK_LAZY) << 24));
      else
        e.tg_list.push_back(e.tgroups[g].slot | (e.tgroups[g].kind << 24));
    }
    for (uint32_t sv = sv_begin[s]; sv < sv_begin[s] + sv_count[s]; sv++) {
      own_off[sv] = (uint32_t)e.tg_list.size();
      for (uint32_t g : e.variants[sv].own) e.tg_list.push_back(g | (selected[g] ? gsd::TL_SELF : 0u));
      own_n[sv] = (uint32_t)e.variants[sv].own.size();
    }
    for (uint32_t g : mine) selected[g] = 0;
  }
  for (uint32_t i = 0; i < e.P; i++) {
    const uint32_t s = spec_of[i];
    for (uint32_t v = e.var_begin[i]; v < e.var_begin[i] + e.var_count[i]; v++) {
      gsd::VarRec& vr = e.vars[v];
      vr.sel_off = sel_off[s];
      vr.sel_n = sel_n[s];
      vr.own_off = own_off[e.var_sv[v]];
      vr.own_n = own_n[e.var_sv[v]];
    }
  }
  if (e.tg_list.empty()) e.tg_list.push_back(0);
}

// per device variant: the lazy groups a pod owns once it relaxes into it
// (the kernels activate them at that Relax)
void Ctx::topo_lazy() {
  e.n_lazy = n_lazy;
  e.lazy_slot.assign(std::max<uint32_t>(n_lazy, 1), 0);
  for (uint32_t g = 0; g < e.TG; g++)
    if (groups[g].lazy)
      e.lazy_slot[groups[g].lazy_idx] = e.tgroups[g].slot | ((e.tgroups[g].kind & gsd::TK_HOST) ? gsd::LZ_HOST : 0u);
  if (n_lazy) {
    // per spec variant its lazy groups (ascending, unique) with its
    // minDomains for each; device variants share their spec variant's run
    std::vector<uint32_t> sv_off(e.variants.size() + 1, 0);
    e.lz_idx.clear();
    e.lz_mind.clear();
    for (size_t sv = 0; sv < e.variants.size(); sv++) {
      auto lm = e.variants[sv].lazy_mind;
      std::sort(lm.begin(), lm.end());
      lm.erase(std::unique(lm.begin(), lm.end(), [](auto& x, auto& y) { return x.first == y.first; }), lm.end());
      sv_off[sv] = (uint32_t)e.lz_idx.size();
      for (auto& x : lm) {
        e.lz_idx.push_back(x.first);
        e.lz_mind.push_back(x.second);
      }
      sv_off[sv + 1] = (uint32_t)e.lz_idx.size();
    }
    // device variant v: [var_lz_off[2v], var_lz_off[2v + 1])
    e.var_lz_off.assign(2 * (size_t)e.V, 0);
    for (uint32_t v = 0; v < e.V; v++) {
      e.var_lz_off[2 * (size_t)v] = sv_off[e.var_sv[v]];
      e.var_lz_off[2 * (size_t)v + 1] = sv_off[e.var_sv[v] + 1];
    }
    if (e.lz_idx.empty()) {
      e.lz_idx.assign(1, 0);
      e.lz_mind.assign(1, 0);
    }
  }
}

// <U> NewTopology: domain universe (In values of NodePool requirements of
// NodePools that have instance types, existing nodes' labels) and the
// counts of the selected bound pods; per variant the owned-group list, per
// pod the selection list (layout.hpp VarRec own_off / sel_off)
void Ctx::build_topology() {
  e.TG = (uint32_t)groups.size();
  e.lazy_slot.assign(1, 0);
  e.var_lz_off.assign(2, 0);
  e.lz_idx.assign(1, 0);
  e.lz_mind.assign(1, 0);
  if (!e.TG) return;
  topo_group_records();
  topo_honor_domains();
  // <U> Topology.AddRequirements intersects every owned group's domains: two
  // groups that pick different domains leave an empty requirement, which a
  // node lacking the domain label passes (strict Compatible: DoesNotExist).
  // The kernels test each group against the node's own domain instead, so
  // such a node beside a pod owning two or more zone-count groups is refused
  if (e.TGZ) {
    bool lacking = false;
    for (auto& nr : e.nodes) lacking = lacking || nr.dvid == gsd::DVID_NONE;
    if (lacking)
      for (auto& pv : e.variants) {
        uint32_t nz = 0;
        for (uint32_t g : pv.own) nz += groups[g].sp.key != kHostname;
        if (nz >= 2)
          throw Fail{GS_E_UNSUPPORTED, "an existing node lacking the " + e.keys[e.k_dom].name +
                                           " label beside a pod owning several topology groups on that key"};
      }
  }
  if (gsd::topo_lds_bytes(e.TGZ, e.ZS, e.TGH, n_lazy) > 64u * 1024u)
    throw Fail{GS_E_UNSUPPORTED, "topology group state exceeds 64 KiB of LDS (zone groups x zones)"};
  e.zcnt0.assign((size_t)std::max<uint32_t>(e.TGZ, 1) * e.ZS, 0);
  e.htot0.assign(std::max<uint32_t>(e.TGH, 1), 0);
  e.hn0.assign((size_t)std::max<uint32_t>(e.TGH, 1) * std::max<uint32_t>(e.NN, 1), 0);
  e.zn_cnt.assign((size_t)std::max<uint32_t>(e.TGZ, 1) * std::max<uint32_t>(e.NN, 1), 0);
  const SelIndex six(groups);
  topo_count_bound(six);
  topo_lists(six);
  topo_lazy();
}

}  // namespace gsh::enc
