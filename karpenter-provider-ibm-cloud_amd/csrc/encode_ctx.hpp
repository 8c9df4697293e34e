// encode_ctx.hpp — internal to the encoder's units (encode.cpp and
// encode_*.cpp): the state one encode() carries from phase to phase, and the
// encoder-side types more than one phase uses.  encode() runs the phases in
// the order they are declared here; each data member names the phase that
// writes it and the later phases that read it.
#pragma once
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "encode.hpp"

namespace gsh::enc {

constexpr const char* kZone = "topology.kubernetes.io/zone";
constexpr const char* kCapacityType = "karpenter.sh/capacity-type";
constexpr const char* kHostname = "kubernetes.io/hostname";
constexpr const char* kNodePool = "karpenter.sh/nodepool";
constexpr const char* kPNS = "PreferNoSchedule";
constexpr const char* kOmega = "\x01<unmentioned>";

// what a phase throws: encode() returns it as the Err
struct Fail {
  gs_status code;
  std::string msg;
};

// GS_ENCODE_PROFILE: wall clock per phase, and per step of the pod phase, on
// stderr (diagnostics)
struct PhaseTimer {
  const bool on = std::getenv("GS_ENCODE_PROFILE") != nullptr;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now(), sub_last = last;
  void phase(const char* name) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "encode %-12s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(t - last).count());
    last = sub_last = t;
  }
  void sub(const char* name) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "  pods.%-18s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(t - sub_last).count());
    sub_last = t;
  }
};

// ------------------------------------------------ topology spread (<U>)
struct SpreadEnc {
  std::string key;
  int32_t skew = 1, mind = 0;
  bool sa = false, has_sel = false, ignore_aff = false, honor_taints = false;
  // <U> TopologyGroup.Hash's node-filter part (oracle/solve.cpp
  // node_filter): taint policy, the filter terms' keys (not their values)
  // and the owner's tolerations; ftext: the terms with their values (a
  // group's owners under AffinityPolicy Honor must agree on it)
  std::string fid, ftext;
  // AffinityPolicy Honor with a filter on more than the zone key: the first
  // owner's filter terms (build_topology applies them to the bound pods'
  // nodes and requires every counted pending spec to carry the same terms)
  bool strict_aff = false;
  std::vector<Reqs> filter;
  std::map<std::string, std::string> ml;
  std::vector<std::tuple<std::string, uint32_t, std::set<std::string>>> ex;
  // metav1.LabelSelector (nil selects nothing)
  bool matches(const std::map<std::string, std::string>& labels) const {
    if (!has_sel) return false;
    for (auto& kv : ml) {
      auto f = labels.find(kv.first);
      if (f == labels.end() || f->second != kv.second) return false;
    }
    for (auto& x : ex) {
      auto f = labels.find(std::get<0>(x));
      const bool present = f != labels.end();
      const uint32_t op = std::get<1>(x);
      const auto& vals = std::get<2>(x);
      if (op == GS_OP_IN && !(present && vals.count(f->second))) return false;
      if (op == GS_OP_NOTIN && present && vals.count(f->second)) return false;
      if (op == GS_OP_EXISTS && !present) return false;
      if (op == GS_OP_DOES_NOT_EXIST && present) return false;
    }
    return true;
  }
  // (minDomains is not part of it: a group keeps its first owner's)
  std::string hash(const std::string& ns) const {
    std::string h = key + "|" + std::to_string(skew) + "|" + ns + "|" + (has_sel ? "1" : "0") +
                    (ignore_aff ? "I" : "H") + (honor_taints ? "H" : "I") + "|f:" + fid;
    for (auto& kv : ml) h += "|l:" + kv.first + "=" + kv.second;
    for (auto& x : ex) {
      h += "|e:" + std::get<0>(x) + ":" + std::to_string(std::get<1>(x));
      for (auto& v : std::get<2>(x)) h += "," + v;
    }
    return h;
  }
};
// <U> corev1.PodAffinityTerm of pod (anti-)affinity (hostname or zone key)
struct AntiEnc {
  SpreadEnc sel;              // key / has_sel / ml / ex
  std::set<std::string> nss;  // the term's namespaces, else the pod's
  bool required = false;
  int32_t weight = 0;
  bool selects(const std::string& ns, const std::map<std::string, std::string>& labels) const {
    return nss.count(ns) && sel.matches(labels);
  }
  std::string hash() const {
    std::string h = "anti|" + sel.key + "|" + std::string(sel.has_sel ? "1" : "0");
    for (auto& n : nss) h += "|n:" + n;
    for (auto& kv : sel.ml) h += "|l:" + kv.first + "=" + kv.second;
    for (auto& x : sel.ex) {
      h += "|e:" + std::get<0>(x) + ":" + std::to_string(std::get<1>(x));
      for (auto& v : std::get<2>(x)) h += "," + v;
    }
    return h;
  }
};
// <U> scheduling.HostPort: Matches = same protocol and port, and either IP
// unspecified or equal (net.ParseIP; unparsable -> 0.0.0.0)
struct PortEnc {
  std::string proto;
  bool unspec = true;
  std::array<uint8_t, 16> ip{};
  int32_t port = 0;
  bool matches(const PortEnc& o) const {
    return proto == o.proto && port == o.port && (unspec || o.unspec || ip == o.ip);
  }
  std::string key() const {
    std::string k = proto + "|" + std::to_string(port) + "|";
    if (!unspec) k.append((const char*)ip.data(), 16);
    return k;
  }
};
// what makes a pod counted by a group
struct PodSel {
  std::string ns;
  std::map<std::string, std::string> labels;
  std::set<std::string> carried;  // hashes of its required anti-affinity terms
  std::vector<PortEnc> ports;
};
// A topology group as the device sees it.  kind 0: a spread constraint
// (counts the pods its selector selects in the owner's namespace).  The
// anti-affinity and host-port constraints are hostname groups whose owner
// may join only a domain with count + self <= skew, self = the owner is
// counted itself; with skew = self that is "count == 0":
//  kind 1 TopologyTypePodAntiAffinity (counts the pods the term selects),
//  kind 2 its inverse for a required term (owners = the pods the term
//         selects; counts the pods carrying the term),
//  kind 3 HostPortUsage (owners = pods with port entry e; counts the pods
//         with an entry that Matches e).
// kind 4 (TopologyTypePodAffinity) counts the pods its term selects and
// admits an owner where count > 0, or, while the total is 0, anywhere if
// the owner is counted itself (tg_aff; the kernel keeps the total).
struct GroupEnc {
  SpreadEnc sp;
  std::string ns;
  int kind = 0;
  AntiEnc anti;
  std::string inv_hash;
  PortEnc port;
  uint32_t owner_spec = gsd::NONE;  // spread groups: the first owner's spec
  // a spread group no pod's first variant keys: Topology.Update creates it
  // when a relaxation first moves a pod to this hash (lazy index; the
  // kernels record into it only once some pod has relaxed into it)
  bool lazy = false;
  uint32_t lazy_idx = 0;
  uint32_t owner_state = 0;         // the first owner's relaxation state (PodWork filter states)
  uint32_t owner_sv = gsd::NONE;    // the first owner's spec variant in that state
};

// Candidate groups of a pod for group_counts: each group is filed under
// one thing a counted pod must carry (a matchLabels pair, a carried term,
// a host port's protocol and number); groups with no such anchor are
// checked for every pod, and nil selectors select nothing
struct SelIndex {
  std::unordered_map<std::string, std::vector<uint32_t>> by;
  std::vector<uint32_t> generic;
  explicit SelIndex(const std::vector<GroupEnc>& gs) {
    for (uint32_t g = 0; g < gs.size(); g++) {
      const GroupEnc& x = gs[g];
      if (x.kind == 2) {
        by["C" + x.inv_hash].push_back(g);
      } else if (x.kind == 3) {
        by["P" + x.port.proto + "|" + std::to_string(x.port.port)].push_back(g);
      } else {
        const SpreadEnc& sel = x.kind == 0 ? x.sp : x.anti.sel;
        if (!sel.has_sel) continue;
        if (!sel.ml.empty()) by["L" + sel.ml.begin()->first + "=" + sel.ml.begin()->second].push_back(g);
        else generic.push_back(g);
      }
    }
  }
  void candidates(const PodSel& ps, std::vector<uint32_t>* out) const {
    *out = generic;
    auto add = [&](const std::string& k) {
      auto f = by.find(k);
      if (f != by.end()) out->insert(out->end(), f->second.begin(), f->second.end());
    };
    if (!by.empty()) {
      for (auto& kv : ps.labels) add("L" + kv.first + "=" + kv.second);
      for (auto& h : ps.carried) add("C" + h);
      for (auto& pe : ps.ports) add("P" + pe.proto + "|" + std::to_string(pe.port));
    }
    std::sort(out->begin(), out->end());
    out->erase(std::unique(out->begin(), out->end()), out->end());
  }
};

// ----------------------------------------------------------- taints
struct TaintKey {
  std::string k, v, eff;
  bool operator<(const TaintKey& o) const { return std::tie(k, v, eff) < std::tie(o.k, o.v, o.eff); }
};
struct Tol {
  std::string k, v, eff;
  uint32_t op;
};
// the pod phase's own types (encode_pods.cpp)
struct PodWork;
struct FilterState;

struct Ctx {
  const gs_problem* p;
  Encoded& e;
  PhaseTimer& tm;
  uint32_t bound_alias;  // bound pod b is also pod bound_alias + b (consolidation); read by build_volumes

  // ------------------------------------------------------------------ data
  // written by encode() (strings) and build_canon, read by every phase
  std::vector<std::string> strs;
  // canonical string ids: the first id carrying each distinct text (callers
  // may repeat a string under several ids)
  std::vector<uint32_t> canon;
  // written by build_vocab (through mention*), read by build_vocab alone
  std::map<std::string, std::set<std::string>> mentions;
  // written by build_catalog, read by build_templates (it_ok), build_pods
  // (rid_map) and, through resvec_fn, build_templates, build_pods, build_nodes
  std::vector<uint64_t> it_ok;
  std::unordered_map<std::string, uint32_t> rid_map;
  std::vector<uint32_t> rid_of_sid;  // string id -> resource index (NONE: not a resource)
  // written by build_templates (taint_id / taint_list also by build_nodes),
  // read by build_pods (tolerate_pns), build_taint_classes, build_topology
  std::vector<std::pair<Reqs, bool>> np_universe;         // NodePool requirements (+labels), has instance types
  std::vector<std::vector<uint32_t>> np_universe_taints;  // per np_universe entry: its taint ids
  std::map<TaintKey, uint32_t> taint_id;
  std::vector<TaintKey> taint_list;
  std::vector<std::vector<uint32_t>> tmpl_taints;  // raw ids per template
  bool tolerate_pns = false;
  // written by choose_shadow_keys, read by build_free_slots
  std::vector<uint32_t> shadow_keys;
  // written by build_pods, read by build_taint_classes (variant_tols) and
  // build_topology (all but group_idx and merge_idx, the pod phase's own)
  // pods -> specs: spec_of[pod], spec_rep[spec] (its first pod), and per spec
  // its variants' range in e.variants (sv_begin / sv_count)
  std::vector<uint32_t> spec_of, spec_rep, sv_begin, sv_count;
  std::vector<PodSel> pod_sel;                        // per pod spec (spec_of)
  std::vector<std::string> spec_aff_text;             // PodWork::aff_text per spec
  std::vector<std::vector<uint32_t>> spec_pref_keys;  // PodWork::pref_keys per spec
  std::vector<std::vector<Tol>> variant_tols;         // per spec variant
  std::vector<GroupEnc> groups;
  std::map<std::string, uint32_t> group_idx;
  // spread groups whose node filter cannot matter (both policies Ignore, or
  // affinity Honor over an empty filter with taints Ignore) and that agree on
  // everything else, minDomains included, count the same pods in the same
  // domains: upstream keeps one group per filter (TopologyGroup.Hash), the
  // product shares one (pod_phase_b)
  std::map<std::string, uint32_t> merge_idx;
  uint32_t n_lazy = 0;
  // written by build_nodes, read by build_taint_classes
  std::vector<std::vector<uint32_t>> node_taints;  // raw ids per node position
  // written by build_taint_classes, read by build_topology
  std::vector<uint64_t> final_sv_tol;
  std::vector<uint32_t> taint_cls;  // taint id -> class

  // ---------------------------------------------------------------- inputs
  const std::string& S(uint32_t id) const {
    if (id >= strs.size()) throw Fail{GS_E_INVALID, "string id out of range"};
    return strs[id];
  }
  uint32_t C(uint32_t id) const {
    if (id >= canon.size()) throw Fail{GS_E_INVALID, "string id out of range"};
    return canon[id];
  }
  void chk(gs_range r, uint32_t n, const char* what) const {
    if ((uint64_t)r.begin + r.count > n) throw Fail{GS_E_INVALID, std::string("range out of bounds: ") + what};
  }

  // ------------------------------------------- vocabulary (encode_vocab.cpp)
  void build_canon();
  void build_vocab();
  void mention(const std::string& key, const std::string& val);
  void mention_key(const std::string& key);
  void mention_reqs(gs_range r);
  void mention_labels(gs_range r);
  uint32_t key_of(uint32_t sid) const;
  KReq kreq_of(const gs_requirement& q) const;
  void no_min_values(gs_range r) const;
  Reqs reqs_of(gs_range r) const;
  KReq in_one(uint32_t key, const std::string& val) const;
  KReq in_one_or_omega(uint32_t key, const std::string& val) const;
  Reqs node_labels_reqs(gs_range r) const;
  Reqs labels_reqs(gs_range r) const;

  // -------------------------- catalog and templates (encode_catalog.cpp)
  void build_catalog();
  void catalog_resources();
  void catalog_thresholds(const std::vector<uint8_t>& ok);
  void resvec_fn(gs_range r, int64_t* out, bool* present) const;
  void build_templates();
  void number_free_keys();
  void choose_shadow_keys();
  void build_free_slots();
  uint64_t zone_has(const Reqs& r) const;
  uint64_t ct_has(const Reqs& r) const;
  uint64_t zone_full(const Reqs& r) const;
  uint32_t zone_flags(const Reqs& r) const;
  uint32_t ct_bits(const Reqs& r);
  uint64_t grid(uint64_t zm, uint64_t cm) const;
  bool it_compat(uint32_t i, const Reqs& r) const;
  gsd::FK to_fk(const KReq& q) const;

  // ------------------------------------------------ pods (encode_pods.cpp)
  // build_pods runs these steps in this order
  void build_pods();
  void pod_specs();
  std::map<std::string, AntiEnc> pod_inverse_terms();
  std::pair<uint32_t, bool> pod_dup_uid() const;
  std::vector<PodWork> pod_spec_work(const std::map<std::string, AntiEnc>& inv_terms, std::pair<uint32_t, bool> dup);
  void pod_variants(std::vector<PodWork> work);
  void pod_var_records();
  void pod_queue_order();
  // a problem without spreads, affinity terms or host ports builds no group:
  // the per-spec selection state (labels, carried terms) is skipped
  bool topo_inputs() const { return p->n_spreads || p->n_affinity_terms || p->n_host_ports; }
  bool pod_sig(const gs_pod& pd, std::vector<uint32_t>& out) const;
  FilterState filter_state(const PodWork& w, size_t ri, const std::vector<Tol>& tols) const;
  void pod_phase_a(uint32_t i, PodWork& w, const std::map<std::string, AntiEnc>& inv_terms);
  void pod_phase_b(uint32_t i, PodWork& w);
  void pod_phase_b2(uint32_t s, PodWork& w);
  void pod_phase_c(PodWork& w);

  // ---------------------------------------------- nodes (encode_nodes.cpp)
  void build_nodes();

  // -------------------------------------------- taints (encode_taints.cpp)
  // the distinct taints of a NodePool / node (raw ids); the device masks are
  // over taint classes (build_taint_classes), so the raw vocabulary may
  // exceed 64
  std::vector<uint32_t> taint_ids(gs_range r, const std::vector<std::pair<std::string, std::string>>* reject = nullptr);
  std::vector<uint32_t> state_taint_ids(const gs_node& g);
  static bool tolerated(const std::vector<Tol>& tols, const TaintKey& tn);
  void build_taint_classes();

  // ----------------------- topology and volumes (encode_topology.cpp)
  std::map<std::string, std::string> label_map(gs_range r) const;
  std::vector<SpreadEnc> spreads_of(const gs_pod& pd) const;
  std::vector<AntiEnc> antis_of(const gs_pod& pd) const;
  std::vector<AntiEnc> terms_of(const gs_pod& pd, gs_range rg, bool affinity) const;
  std::vector<PortEnc> ports_of(const gs_pod& pd) const;
  PodSel sel_of(const gs_pod& pd) const;
  bool group_counts(const GroupEnc& g, const PodSel& ps) const;
  uint32_t group_id(const std::string& h, GroupEnc&& g);
  GroupEnc host_group(int kind, bool self, const std::string& key = kHostname) const;
  // build_topology runs these steps in this order
  void build_topology();
  void topo_group_records();
  void topo_honor_domains();
  void topo_count_bound(const SelIndex& six);
  void topo_lists(const SelIndex& six);
  void topo_lazy();
  void build_volumes();
};

}  // namespace gsh::enc
