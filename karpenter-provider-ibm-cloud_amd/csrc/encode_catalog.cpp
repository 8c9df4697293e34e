// encode_catalog.cpp — the encoder's catalog and template phases: instance
// types, offerings and resources; NodePools -> NodeClaim templates; the free
// requirement-key slots (shadow keys among them).
#include "encode_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <set>

namespace gsh::enc {

// ----------------------------------------------------------- catalog
// the resource names in sorted order (resource index), and each quantity's
// string id -> resource index
void Ctx::catalog_resources() {
  // (canonical string ids of the resource names: the first id carrying
  // each text, so a resource's lowest string id is its canonical id)
  std::set<std::string> rn;
  std::vector<uint32_t> res_cids;
  {
    std::vector<uint8_t> seen(strs.size(), 0);
    for (uint32_t i = 0; i < p->n_quantities; i++) {
      const uint32_t c = C(p->quantities[i].resource);
      if (!seen[c]) {
        seen[c] = 1;
        rn.insert(strs[c]);
        res_cids.push_back(c);
      }
    }
  }
  e.res_names.assign(rn.begin(), rn.end());
  e.R = (uint32_t)e.res_names.size();
  if (e.R > (uint32_t)gsd::RMAX) throw Fail{GS_E_UNSUPPORTED, "more than 8 distinct resources"};
  std::unordered_map<std::string, uint32_t> rid;
  for (uint32_t r = 0; r < e.R; r++) rid[e.res_names[r]] = r;
  e.res_name_ids.assign(e.R, 0);
  std::vector<uint32_t> rid_of_cid(res_cids.size());
  for (size_t k = 0; k < res_cids.size(); k++) {
    const uint32_t r = rid.at(strs[res_cids[k]]);
    e.res_name_ids[r] = res_cids[k];
    rid_of_cid[k] = r;
  }
  rid_map = rid;
  // string id -> resource index for every string a quantity names (the
  // only ids resvec_fn looks up)
  rid_of_sid.assign(strs.size(), gsd::NONE);
  {
    std::unordered_map<uint32_t, uint32_t> by_cid;
    for (size_t k = 0; k < res_cids.size(); k++) by_cid[res_cids[k]] = rid_of_cid[k];
    for (uint32_t i = 0; i < p->n_quantities; i++) {
      const uint32_t sid = p->quantities[i].resource;
      if (rid_of_sid[sid] == gsd::NONE) rid_of_sid[sid] = by_cid.at(C(sid));
    }
  }
}

void Ctx::build_catalog() {
  e.N = p->n_instance_types;
  e.W = (e.N + 63) / 64;
  if (e.N == 0) throw Fail{GS_E_INVALID, "empty catalog"};
  // IT keys: the key set of IT 0; every IT must carry exactly those keys,
  // each single-valued In (reference instancetype.go:721-726)
  std::vector<uint32_t> k0;
  for (uint32_t i = 0; i < e.N; i++) {
    auto& it = p->instance_types[i];
    std::vector<uint32_t> ks;
    for (uint32_t k = 0; k < it.requirements.count; k++) {
      auto& q = p->reqs[it.requirements.begin + k];
      if (q.op != GS_OP_IN || q.values.count != 1)
        throw Fail{GS_E_UNSUPPORTED, "instance type requirement is not single-valued In"};
      ks.push_back(key_of(q.key));
    }
    std::sort(ks.begin(), ks.end());
    if (std::adjacent_find(ks.begin(), ks.end()) != ks.end())
      throw Fail{GS_E_UNSUPPORTED, "instance type repeats a requirement key"};
    if (i == 0) k0 = ks;
    else if (ks != k0) throw Fail{GS_E_UNSUPPORTED, "instance types carry different requirement keys"};
  }
  for (auto k : k0) {
    if (k == e.k_zone || k == e.k_ct || k == e.k_hostname)
      throw Fail{GS_E_UNSUPPORTED, "instance type requirement on zone/capacity-type/hostname"};
    e.keys[k].cls = KEY_IT;
    e.keys[k].slot = (int)e.it_keys.size();
    e.it_keys.push_back(k);
  }
  e.K = (uint32_t)e.it_keys.size();
  if (e.K > (uint32_t)gsd::KMAX_IT) throw Fail{GS_E_UNSUPPORTED, "too many instance-type keys"};
  e.keys[e.k_zone].cls = KEY_ZONE;
  e.keys[e.k_ct].cls = KEY_CT;
  // catalog zones / capacity types in first-appearance order
  std::map<uint32_t, uint32_t> zmap, cmap;
  struct Off {
    uint32_t z, c;
    double price;
    bool avail;
  };
  std::vector<std::vector<Off>> offs(e.N);
  for (uint32_t i = 0; i < e.N; i++) {
    auto& it = p->instance_types[i];
    if (it.offerings.count > (uint32_t)gsd::SMAX) throw Fail{GS_E_UNSUPPORTED, "too many offerings per instance type"};
    for (uint32_t s = 0; s < it.offerings.count; s++) {
      auto& o = p->offerings[it.offerings.begin + s];
      uint32_t zv = gsd::NONE, cv = gsd::NONE;
      for (uint32_t k = 0; k < o.requirements.count; k++) {
        auto& q = p->reqs[o.requirements.begin + k];
        uint32_t key = key_of(q.key);
        if (q.op != GS_OP_IN || q.values.count != 1) throw Fail{GS_E_UNSUPPORTED, "offering requirement not single In"};
        uint32_t vid = e.keys[key].vocab.id.at(S(p->value_ids[q.values.begin]));
        if (key == e.k_zone && zv == gsd::NONE) zv = vid;
        else if (key == e.k_ct && cv == gsd::NONE) cv = vid;
        else throw Fail{GS_E_UNSUPPORTED, "offering requirements other than one zone and one capacity type"};
      }
      if (zv == gsd::NONE || cv == gsd::NONE) throw Fail{GS_E_UNSUPPORTED, "offering without zone or capacity type"};
      if (std::isnan(o.price)) throw Fail{GS_E_UNSUPPORTED, "NaN offering price"};
      if (!zmap.count(zv)) {
        uint32_t n = (uint32_t)zmap.size();
        zmap[zv] = n;
        e.cat_zone.push_back(zv);
      }
      if (!cmap.count(cv)) {
        uint32_t n = (uint32_t)cmap.size();
        cmap[cv] = n;
        e.cat_ct.push_back(cv);
      }
      offs[i].push_back({zmap[zv], cmap[cv], o.price, o.available != 0});
    }
  }
  e.Z = (uint32_t)e.cat_zone.size();
  e.C = (uint32_t)e.cat_ct.size();
  if (e.Z * e.C > 64) throw Fail{GS_E_UNSUPPORTED, "zones x capacity types > 64"};
  catalog_resources();
  // per IT arrays
  e.it_vid.assign((size_t)e.K * e.N, 0);
  e.it_alloc.assign((size_t)e.R * e.N, 0);
  e.it_cap.assign((size_t)e.R * e.N, 0);
  e.it_pair.assign(e.N, 0);
  e.it_prank.assign((size_t)e.N * 64, gsd::NONE);
  // price ranks
  std::vector<double> prices;
  for (auto& v : offs)
    for (auto& o : v) prices.push_back(o.price);
  std::sort(prices.begin(), prices.end());
  prices.erase(std::unique(prices.begin(), prices.end(), [](double a, double b) { return a == b; }), prices.end());
  e.prices = prices;
  auto prank = [&](double x) {
    return (uint32_t)(std::lower_bound(prices.begin(), prices.end(), x) - prices.begin());
  };
  std::vector<uint8_t> ok(e.N, 1);
  for (uint32_t i = 0; i < e.N; i++) {
    auto& it = p->instance_types[i];
    for (uint32_t k = 0; k < it.requirements.count; k++) {
      auto& q = p->reqs[it.requirements.begin + k];
      uint32_t key = key_of(q.key);
      e.it_vid[(size_t)e.keys[key].slot * e.N + i] = e.keys[key].vocab.id.at(S(p->value_ids[q.values.begin]));
    }
    int64_t cap[gsd::RMAX] = {0}, ovh[gsd::RMAX] = {0};
    bool capp[gsd::RMAX] = {false}, ovhp[gsd::RMAX] = {false};
    resvec_fn(it.capacity, cap, capp);
    resvec_fn(it.overhead, ovh, ovhp);
    for (uint32_t r = 0; r < e.R; r++) {
      // Allocatable = Subtract(Capacity, Overhead.Total()) over capacity keys
      int64_t a = capp[r] ? cap[r] - (ovhp[r] ? ovh[r] : 0) : 0;
      e.it_alloc[(size_t)r * e.N + i] = a;
      e.it_cap[(size_t)r * e.N + i] = cap[r];
      if (capp[r] && a < 0) ok[i] = 0;  // <U> Fits: any negative total never fits
    }
    uint64_t seen = 0;
    for (auto& o : offs[i]) {
      uint32_t g = o.z * e.C + o.c;
      if (seen >> g & 1) throw Fail{GS_E_UNSUPPORTED, "instance type repeats a (zone, capacity type) offering"};
      seen |= 1ull << g;
      if (o.avail) {
        e.it_pair[i] |= 1ull << g;
        e.it_prank[(size_t)i * 64 + g] = prank(o.price);
      }
    }
    if (!ok[i]) e.it_pair[i] = 0;  // never selectable
  }
  it_ok.assign(e.W, 0);
  for (uint32_t i = 0; i < e.N; i++)
    if (ok[i]) it_ok[i / 64] |= 1ull << (i % 64);
  // name ranks (Go string order = bytewise)
  std::vector<uint32_t> order(e.N);
  std::iota(order.begin(), order.end(), 0);
  std::vector<std::string> names(e.N);
  for (uint32_t i = 0; i < e.N; i++) names[i] = S(p->instance_types[i].name);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
  for (uint32_t i = 0; i + 1 < e.N; i++)
    if (names[order[i]] == names[order[i + 1]]) throw Fail{GS_E_INVALID, "duplicate instance type name"};
  e.it_namerank.assign(e.N, 0);
  e.rank_to_it = order;
  for (uint32_t r = 0; r < e.N; r++) e.it_namerank[order[r]] = r;
  // slot sets
  e.slot_set.assign((size_t)64 * e.W, 0);
  for (uint32_t i = 0; i < e.N; i++)
    for (uint32_t g = 0; g < 64; g++)
      if (e.it_pair[i] >> g & 1) e.slot_set[(size_t)g * e.W + i / 64] |= 1ull << (i % 64);
  catalog_thresholds(ok);
}

// fit thresholds per resource over selectable ITs (`ok`)
void Ctx::catalog_thresholds(const std::vector<uint8_t>& ok) {
  e.thr_off.assign(e.R + 1, 0);
  std::vector<std::vector<int64_t>> vals(e.R);
  for (uint32_t r = 0; r < e.R; r++) {
    for (uint32_t i = 0; i < e.N; i++)
      if (ok[i]) vals[r].push_back(e.it_alloc[(size_t)r * e.N + i]);
    std::sort(vals[r].begin(), vals[r].end());
    vals[r].erase(std::unique(vals[r].begin(), vals[r].end()), vals[r].end());
    e.thr_off[r + 1] = e.thr_off[r] + (uint32_t)vals[r].size();
  }
  e.thr_val.clear();
  for (uint32_t r = 0; r < e.R; r++) e.thr_val.insert(e.thr_val.end(), vals[r].begin(), vals[r].end());
  // thr_set: for resource r, m in [0, n_r]: rows at (thr_off[r] + r + m)
  e.thr_set.assign((size_t)(e.thr_off[e.R] + e.R) * e.W, 0);
  for (uint32_t r = 0; r < e.R; r++)
    for (uint32_t m = 0; m < vals[r].size(); m++) {
      uint64_t* row = &e.thr_set[(size_t)(e.thr_off[r] + r + m) * e.W];
      for (uint32_t i = 0; i < e.N; i++)
        if (ok[i] && e.it_alloc[(size_t)r * e.N + i] >= vals[r][m]) row[i / 64] |= 1ull << (i % 64);
    }
}

void Ctx::resvec_fn(gs_range r, int64_t* out, bool* present) const {
  chk(r, p->n_quantities, "quantities");
  for (uint32_t k = 0; k < r.count; k++) {
    auto& q = p->quantities[r.begin + k];
    if (q.resource >= rid_of_sid.size() || rid_of_sid[q.resource] == gsd::NONE)
      throw Fail{GS_E_INVALID, "unknown resource"};
    const uint32_t x = rid_of_sid[q.resource];
    out[x] += q.milli;
    if (present) present[x] = true;
  }
}

// ----------------------------------------------------- helpers on Reqs
uint64_t Ctx::zone_has(const Reqs& r) const {
  auto it = r.find(e.k_zone);
  uint64_t m = 0;
  for (uint32_t z = 0; z < e.Z; z++)
    if (it == r.end() || it->second.has.test(e.cat_zone[z])) m |= 1ull << z;
  return m;
}
uint64_t Ctx::ct_has(const Reqs& r) const {
  auto it = r.find(e.k_ct);
  uint64_t m = 0;
  for (uint32_t c = 0; c < e.C; c++)
    if (it == r.end() || it->second.has.test(e.cat_ct[c])) m |= 1ull << c;
  return m;
}
// zone Has over the zone vocabulary (first word; topology needs <= 64
// values) and the complement flag of the zone requirement
uint64_t Ctx::zone_full(const Reqs& r) const {
  auto f = r.find(e.k_dom);
  return f == r.end() ? ~0ull : f->second.has.w[0];
}
uint32_t Ctx::zone_flags(const Reqs& r) const {
  auto f = r.find(e.k_dom);
  return f == r.end() || f->second.comp ? gsd::ZF_COMP : 0u;
}

// CT_SPOT | CT_OD: Requirement.Has("spot") / Has("on-demand") of the
// capacity-type key (an absent key is Exists: both); values nobody
// mentions behave like omega
uint32_t Ctx::ct_bits(const Reqs& r) {
  auto f = r.find(e.k_ct);
  if (f == r.end()) return gsd::CT_SPOT | gsd::CT_OD;
  const Vocab& v = e.keys[e.k_ct].vocab;
  auto vid = [&](const char* x) {
    auto g = v.id.find(x);
    return g == v.id.end() ? v.omega : g->second;
  };
  return (f->second.has.test(vid("spot")) ? gsd::CT_SPOT : 0u) | (f->second.has.test(vid("on-demand")) ? gsd::CT_OD : 0u);
}

uint64_t Ctx::grid(uint64_t zm, uint64_t cm) const {
  uint64_t g = 0;
  for (uint32_t z = 0; z < e.Z; z++)
    if (zm >> z & 1) g |= (cm & ((1ull << e.C) - 1)) << (z * e.C);
  return g;
}
// compat(IT, reqs) over IT keys: <U> it.Requirements.Intersects(reqs)
bool Ctx::it_compat(uint32_t i, const Reqs& r) const {
  for (uint32_t k = 0; k < e.K; k++) {
    auto f = r.find(e.it_keys[k]);
    if (f == r.end()) continue;
    if (!f->second.has.test(e.it_vid[(size_t)k * e.N + i])) return false;
  }
  return true;
}
gsd::FK Ctx::to_fk(const KReq& q) const {
  gsd::FK f{};
  for (int i = 0; i < gsd::FKW; i++) {
    f.has[i] = i < (int)q.has.w.size() ? q.has.w[i] : 0;
    f.excl[i] = i < (int)q.excl.w.size() ? q.excl.w[i] : 0;
  }
  f.gt = q.gt;
  f.lt = q.lt;
  f.flags = gsd::FK_PRESENT | (q.comp ? gsd::FK_COMP : 0) | (q.hg ? gsd::FK_GT : 0) | (q.hl ? gsd::FK_LT : 0);
  return f;
}

void Ctx::build_templates() {
  // dense per-key value ids of the catalog (minValues counting)
  e.it_dvid.assign((size_t)e.K * e.N, 0);
  e.it_ndv.assign(e.K, 0);
  for (uint32_t k = 0; k < e.K; k++) {
    std::map<uint32_t, uint16_t> dense;
    for (uint32_t i = 0; i < e.N; i++) {
      auto f = dense.emplace(e.it_vid[(size_t)k * e.N + i], (uint16_t)std::min<size_t>(dense.size(), 65535)).first;
      e.it_dvid[(size_t)k * e.N + i] = f->second;
    }
    e.it_ndv[k] = (uint32_t)dense.size();
    if (dense.size() == e.N) e.it_key_unique |= 1u << k;
  }
  std::vector<uint32_t> order(p->n_nodepools);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    auto& A = p->nodepools[a];
    auto& B = p->nodepools[b];
    if (A.weight == B.weight) return S(A.name) < S(B.name);
    return A.weight > B.weight;
  });
  for (uint32_t npi : order) {
    auto& np = p->nodepools[npi];
    Reqs npreqs = reqs_of(np.requirements);
    // NewNodeClaimTemplate: spec requirements + labels + nodepool label
    Reqs tr = npreqs;
    std::map<std::string, std::string> labels;
    for (uint32_t i = 0; i < np.labels.count; i++)
      labels[S(p->labels[np.labels.begin + i].key)] = S(p->labels[np.labels.begin + i].value);
    labels[kNodePool] = S(np.name);
    for (auto& kv : labels) {
      uint32_t k = e.key_id.at(label_normalize(kv.first));
      reqs_add(e, tr, k, in_one(k, kv.second));
    }
    uint64_t zm = zone_has(tr), cm = ct_has(tr), G = grid(zm, cm);
    // GetInstanceTypes filter + NewScheduler pre-filter (compat, fits({}), offering)
    chk(np.instance_types, p->n_it_refs, "it_refs");
    for (uint32_t k = 0; k < np.instance_types.count; k++) {
      uint32_t i = p->it_refs[np.instance_types.begin + k];
      if (i < e.N) e.checks_per_pod += p->instance_types[i].offerings.count;
    }
    std::vector<uint64_t> opts(e.W, 0);
    bool any = false, has_its = false;
    for (uint32_t k = 0; k < np.instance_types.count; k++) {
      uint32_t i = p->it_refs[np.instance_types.begin + k];
      if (i >= e.N) throw Fail{GS_E_INVALID, "it_ref out of range"};
      Reqs itr;
      for (uint32_t kk = 0; kk < e.K; kk++)
        itr.emplace(e.it_keys[kk], in_one(e.it_keys[kk], e.keys[e.it_keys[kk]].vocab.vals[e.it_vid[(size_t)kk * e.N + i]]));
      if (!reqs_compatible(e, npreqs, itr, true)) continue;
      has_its = true;  // CloudProvider.GetInstanceTypes keeps it (topology universe)
      if (!(it_ok[i / 64] >> (i % 64) & 1)) continue;
      if (!it_compat(i, tr)) continue;
      if (!(e.it_pair[i] & G)) continue;
      opts[i / 64] |= 1ull << (i % 64);
      any = true;
    }
    std::vector<uint32_t> tm = taint_ids(np.taints);
    np_universe.emplace_back(tr, has_its);
    np_universe_taints.push_back(tm);
    // <U> minValues (Strict): NewScheduler's filterInstanceTypesByRequirements
    // drops the NodePool when its options miss a minimum.  Instance types
    // carry no value for a key outside the IT keys (Values() is empty).
    uint32_t mv_mask = 0;
    uint16_t mvk[gsd::KMAX_IT] = {0};
    for (auto& kv : tr) {
      if (kv.second.mv <= 0) continue;
      if (e.keys[kv.first].cls != KEY_IT) {
        any = false;
        continue;
      }
      const int ks = e.keys[kv.first].slot;
      if (!((e.it_key_unique >> ks) & 1) && e.it_ndv[ks] > 256)
        throw Fail{GS_E_UNSUPPORTED, "minValues on a key with more than 256 instance-type values"};
      mv_mask |= 1u << ks;
      mvk[ks] = (uint16_t)std::min<int64_t>(kv.second.mv, 65535);
      std::set<uint32_t> vals;
      for (uint32_t i = 0; i < e.N; i++)
        if ((opts[i / 64] >> (i % 64)) & 1) vals.insert(e.it_vid[(size_t)ks * e.N + i]);
      if ((int64_t)vals.size() < kv.second.mv) any = false;
    }
    if (!any) continue;
    if (e.T >= (uint32_t)gsd::TMAX) throw Fail{GS_E_UNSUPPORTED, "more than 64 NodePools"};
    gsd::TmplRec t{};
    t.np_index = npi;
    t.zm = zm;
    t.cm = cm;
    t.taints = 0;  // build_taint_classes
    bool present[gsd::RMAX] = {false};
    resvec_fn(np.daemon_requests, t.daemon, nullptr);
    if (np.has_limits) {
      t.has_limits = 1;
      resvec_fn(np.limits, t.limits, present);
      for (uint32_t r = 0; r < e.R; r++)
        if (present[r]) t.limit_rmask |= 1u << r;
    }
    for (uint32_t i = 0; i < np.taints.count; i++)
      if (S(p->taints[np.taints.begin + i].effect) == kPNS) tolerate_pns = true;
    // NewNodeClaim adds hostname In[placeholder]
    reqs_add(e, tr, e.k_hostname, make_kreq(e.keys[e.k_hostname].vocab, GS_OP_IN, {e.keys[e.k_hostname].vocab.omega}, 0));
    t.ctb = ct_bits(tr);
    {
      // the static matrix folds NodePool limits in: filterByRemainingResources
      std::vector<uint64_t> lim = opts;
      if (t.has_limits)
        for (uint32_t i = 0; i < e.N; i++) {
          if (!(lim[i / 64] >> (i % 64) & 1)) continue;
          for (uint32_t r = 0; r < e.R; r++)
            if ((t.limit_rmask >> r & 1) && e.it_cap[(size_t)r * e.N + i] > t.limits[r]) lim[i / 64] &= ~(1ull << (i % 64));
        }
      e.t_limopts.insert(e.t_limopts.end(), lim.begin(), lim.end());
    }
    t.zfull = zone_full(tr);
    t.zflags = zone_flags(tr);
    t.mv_mask = mv_mask;
    for (int k = 0; k < gsd::KMAX_IT; k++) t.mv[k] = mvk[k];
    if (mv_mask) e.any_mv = true;
    e.tmpl.push_back(t);
    tmpl_taints.push_back(std::move(tm));
    e.t_opts.insert(e.t_opts.end(), opts.begin(), opts.end());
    e.tmpl_reqs.push_back(tr);
    e.T++;
  }
}

// --------------------------------------------------------------- pods
// <U> ExistingNode.CanAdd: a node lacking a label satisfies a pod's
// NotIn / DoesNotExist on it (Requirements.Compatible), and Add then gives
// the node a requirement on that key, which later pods meet by intersection.
// Instance-type, zone and capacity-type keys hold a node's label as one
// value id; where some node lacks such a key that some pod term constrains
// with NotIn / DoesNotExist, the key also gets a free slot ("shadow") that
// carries the nodes' full requirement state, and the node check runs on it
// instead of the value id.  Claims keep their own checks (the shadow entry
// is a redundant, well-known free key there).  Not for a zone key that
// topology counts on (a node's zone domain comes from its label).
void Ctx::choose_shadow_keys() {
  if (!p->n_nodes) return;
  std::set<uint32_t> constrained;
  // every key a pod's node selector or terms mention: a variant's
  // requirement can come out NotIn / DoesNotExist from In / Gt / Lt terms
  // too (an empty intersection is DoesNotExist)
  auto scan = [&](const gs_pod* pods, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
      const gs_range sr = pods[i].node_selector;
      chk(sr, p->n_labels, "labels");
      for (uint32_t j = 0; j < sr.count; j++) constrained.insert(key_of(p->labels[sr.begin + j].key));
      for (gs_range tr : {pods[i].required_terms, pods[i].preferred_terms}) {
        chk(tr, p->n_terms, "terms");
        for (uint32_t t = 0; t < tr.count; t++) {
          const gs_range rr = p->terms[tr.begin + t].requirements;
          chk(rr, p->n_reqs, "reqs");
          for (uint32_t q = 0; q < rr.count; q++) constrained.insert(key_of(p->reqs[rr.begin + q].key));
        }
      }
    }
  };
  scan(p->pods, p->n_pods);
  if (p->bound_pods) scan(p->bound_pods, p->n_bound_pods);
  bool zone_topology = false;
  for (uint32_t i = 0; i < p->n_spreads; i++) zone_topology = zone_topology || label_normalize(S(p->spreads[i].topology_key)) == kZone;
  for (uint32_t i = 0; i < p->n_affinity_terms; i++)
    zone_topology = zone_topology || label_normalize(S(p->affinity_terms[i].topology_key)) == kZone;
  for (uint32_t k : constrained) {
    Key& key = e.keys[k];
    if (key.cls == KEY_FREE || !key.wellknown || key.vocab.size() > (size_t)gsd::FKV) continue;
    if (key.cls == KEY_ZONE && zone_topology) continue;
    if (key.cls == KEY_CT && e.dom_ct) continue;
    bool lacking = false;
    for (uint32_t i = 0; i < p->n_nodes && !lacking; i++) {
      const gs_range lr = p->nodes[i].labels;
      chk(lr, p->n_labels, "labels");
      bool has = false;
      for (uint32_t j = 0; j < lr.count && !has; j++) has = key_of(p->labels[lr.begin + j].key) == k;
      lacking = !has;
    }
    if (lacking) shadow_keys.push_back(k);
  }
}

// the free keys' slots, in key order (before choose_shadow_keys: its errors come second)
void Ctx::number_free_keys() {
  for (uint32_t k = 0; k < e.keys.size(); k++) {
    if (e.keys[k].cls != KEY_FREE) continue;
    if (e.keys[k].vocab.size() > (size_t)gsd::FKV)
      throw Fail{GS_E_UNSUPPORTED, "free key vocabulary > 255 values: " + e.keys[k].name};
    if (e.free_keys.size() >= (size_t)gsd::FMAX) throw Fail{GS_E_UNSUPPORTED, "more than 16 free requirement keys"};
    e.keys[k].slot = (int)e.free_keys.size();
    if (e.keys[k].wellknown) e.wk_slots |= 1ull << e.free_keys.size();
    e.free_keys.push_back(k);
  }
}

// the shadow keys' slots after them, then the device's free-key tables
void Ctx::build_free_slots() {
  for (uint32_t k : shadow_keys) {
    if (e.free_keys.size() >= (size_t)gsd::FMAX) break;  // build_nodes refuses what stays unshadowed
    e.keys[k].shadow = (int)e.free_keys.size();
    e.wk_slots |= 1ull << e.free_keys.size();
    e.free_keys.push_back(k);
  }
  e.F = (uint32_t)e.free_keys.size();
  e.fk_ival.assign((size_t)std::max<uint32_t>(e.F, 1) * gsd::FKV, 0);
  e.fk_isint.assign((size_t)std::max<uint32_t>(e.F, 1) * gsd::FKW, 0);
  for (uint32_t s = 0; s < e.F; s++) {
    auto& v = e.keys[e.free_keys[s]].vocab;
    for (uint32_t i = 0; i < v.size(); i++) {
      e.fk_ival[(size_t)s * gsd::FKV + i] = v.ival[i];
      if (v.isint[i]) e.fk_isint[(size_t)s * gsd::FKW + i / 64] |= 1ull << (i % 64);
    }
  }
  e.t_fk.assign((size_t)e.T * std::max<uint32_t>(e.F, 1), gsd::FK{});
  for (uint32_t t = 0; t < e.T; t++)
    for (auto& kv : e.tmpl_reqs[t]) {
      const Key& key = e.keys[kv.first];
      if (key.cls == KEY_FREE || key.shadow >= 0)
        e.t_fk[(size_t)t * e.F + (key.cls == KEY_FREE ? key.slot : key.shadow)] = to_fk(kv.second);
    }
}

}  // namespace gsh::enc
