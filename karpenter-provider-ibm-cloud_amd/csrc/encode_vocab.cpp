// encode_vocab.cpp — the encoder's vocabulary phase: canonical string ids, the
// per-key value vocabularies, and gs_requirement / labels -> Reqs over them.
#include "encode_ctx.hpp"

#include <climits>
#include <set>
#include <string_view>

namespace gsh::enc {

void Ctx::build_canon() {
  const uint32_t n = (uint32_t)strs.size();
  canon.resize(n);
  // strings hashed in parallel, then each shard's first-id map built by its
  // own thread over its ids in ascending order
  const uint32_t SH = 64;
  std::vector<uint64_t> hs(n);
  par_for(n, 4096, [&](uint32_t i) { hs[i] = std::hash<std::string_view>{}(std::string_view(strs[i])); });
  std::vector<uint32_t> cnt(SH + 1, 0), ids(n);
  for (uint32_t i = 0; i < n; i++) cnt[hs[i] % SH + 1]++;
  for (uint32_t k = 0; k < SH; k++) cnt[k + 1] += cnt[k];
  {
    std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
    for (uint32_t i = 0; i < n; i++) ids[fill[hs[i] % SH]++] = i;
  }
  par_for(SH, 1, [&](uint32_t k) {
    std::unordered_map<std::string_view, uint32_t> first;
    first.reserve((cnt[k + 1] - cnt[k]) * 2);
    for (uint32_t x = cnt[k]; x < cnt[k + 1]; x++) {
      const uint32_t i = ids[x];
      canon[i] = first.emplace(std::string_view(strs[i]), i).first->second;
    }
  });
}

void Ctx::mention(const std::string& key, const std::string& val) { mentions[label_normalize(key)].insert(val); }
void Ctx::mention_key(const std::string& key) { mentions[label_normalize(key)]; }
void Ctx::mention_reqs(gs_range r) {
  chk(r, p->n_reqs, "reqs");
  for (uint32_t i = 0; i < r.count; i++) {
    auto& q = p->reqs[r.begin + i];
    if (q.op > GS_OP_LTE) throw Fail{GS_E_INVALID, "unknown requirement operator"};
    chk(q.values, p->n_value_ids, "values");
    mention_key(S(q.key));
    if (q.op == GS_OP_IN || q.op == GS_OP_NOTIN)
      for (uint32_t k = 0; k < q.values.count; k++) {
        const std::string& v = S(p->value_ids[q.values.begin + k]);
        if (label_normalize(S(q.key)) == kHostname && v.rfind("hostname-placeholder-", 0) == 0)
          throw Fail{GS_E_UNSUPPORTED, "requirement names a hostname placeholder"};
        mention(S(q.key), v);
      }
    if (q.op >= GS_OP_GT) {
      int64_t x;
      if (q.values.count < 1 || !go_atoi64(S(p->value_ids[q.values.begin]), &x))
        throw Fail{GS_E_INVALID, "Gt/Lt/Gte/Lte value is not an integer"};
      if ((q.op == GS_OP_GTE && x == INT64_MIN) || (q.op == GS_OP_LTE && x == INT64_MAX))
        throw Fail{GS_E_INVALID, "Gte/Lte bound out of range"};
    }
  }
}
void Ctx::mention_labels(gs_range r) {
  chk(r, p->n_labels, "labels");
  for (uint32_t i = 0; i < r.count; i++) mention(S(p->labels[r.begin + i].key), S(p->labels[r.begin + i].value));
}

void Ctx::build_vocab() {
  mention_key(kZone);
  mention_key(kCapacityType);
  mention_key(kHostname);
  mention_key(kNodePool);
  for (uint32_t i = 0; i < p->n_instance_types; i++) {
    auto& it = p->instance_types[i];
    mention_reqs(it.requirements);
    chk(it.offerings, p->n_offerings, "offerings");
    for (uint32_t k = 0; k < it.offerings.count; k++) mention_reqs(p->offerings[it.offerings.begin + k].requirements);
  }
  for (uint32_t i = 0; i < p->n_nodepools; i++) {
    auto& np = p->nodepools[i];
    mention_reqs(np.requirements);
    mention_labels(np.labels);
    mention(kNodePool, S(np.name));
  }
  // node label values matter only where a requirement can tell them apart:
  // on instance-type / offering keys, or as integers under Gt/Lt bounds.
  // Any other value behaves exactly like the unmentioned value omega.
  std::set<std::string> label_keys = {kZone, kCapacityType}, bounded;
  // a NodePool-key spread tells nodes of unknown NodePools apart (domains)
  for (uint32_t i = 0; i < p->n_spreads; i++)
    if (label_normalize(S(p->spreads[i].topology_key)) == kNodePool) label_keys.insert(kNodePool);
  if (p->n_instance_types) {
    auto& it0 = p->instance_types[0];
    chk(it0.requirements, p->n_reqs, "reqs");
    for (uint32_t k = 0; k < it0.requirements.count; k++)
      label_keys.insert(label_normalize(S(p->reqs[it0.requirements.begin + k].key)));
  }
  for (uint32_t i = 0; i < p->n_reqs; i++)
    if (p->reqs[i].op >= GS_OP_GT && p->reqs[i].op <= GS_OP_LTE) bounded.insert(label_normalize(S(p->reqs[i].key)));
  auto node_mention = [&](const std::string& key, const std::string& val) {
    const std::string k = label_normalize(key);
    int64_t x;
    if (label_keys.count(k) || (bounded.count(k) && go_atoi64(val, &x))) mention(k, val);
    else mention_key(k);
  };
  for (uint32_t i = 0; i < p->n_nodes; i++) {
    chk(p->nodes[i].labels, p->n_labels, "labels");
    for (uint32_t k = 0; k < p->nodes[i].labels.count; k++)
      node_mention(S(p->labels[p->nodes[i].labels.begin + k].key), S(p->labels[p->nodes[i].labels.begin + k].value));
    node_mention(kHostname, S(p->nodes[i].name));
  }
  for (uint32_t i = 0; i < p->n_pods; i++) {
    auto& pd = p->pods[i];
    mention_labels(pd.node_selector);
    chk(pd.required_terms, p->n_terms, "terms");
    chk(pd.preferred_terms, p->n_terms, "terms");
    for (uint32_t k = 0; k < pd.required_terms.count; k++) mention_reqs(p->terms[pd.required_terms.begin + k].requirements);
    for (uint32_t k = 0; k < pd.preferred_terms.count; k++)
      mention_reqs(p->terms[pd.preferred_terms.begin + k].requirements);
  }
  for (auto& kv : mentions) {
    Key k;
    k.name = kv.first;
    k.wellknown = label_is_wellknown(kv.first);
    for (auto& v : kv.second) {
      k.vocab.id[v] = (uint32_t)k.vocab.vals.size();
      k.vocab.vals.push_back(v);
    }
    k.vocab.omega = (uint32_t)k.vocab.vals.size();
    k.vocab.vals.push_back(kOmega);
    for (auto& v : k.vocab.vals) {
      int64_t x = 0;
      bool ok = v != kOmega && go_atoi64(v, &x);
      k.vocab.isint.push_back(ok);
      k.vocab.ival.push_back(x);
    }
    e.key_id[k.name] = (uint32_t)e.keys.size();
    e.keys.push_back(std::move(k));
  }
  e.k_zone = e.key_id[kZone];
  e.k_ct = e.key_id[kCapacityType];
  e.k_hostname = e.key_id[kHostname];
  e.k_nodepool = e.key_id[kNodePool];
  // spreads on the capacity-type key move the domain machinery onto it
  // (build_nodes / build_pods swap the zone and capacity-type fields)
  e.dom_ct = e.dom_np = false;
  for (uint32_t i = 0; i < p->n_spreads; i++) {
    const std::string k = label_normalize(S(p->spreads[i].topology_key));
    e.dom_ct = e.dom_ct || k == kCapacityType;
    e.dom_np = e.dom_np || k == kNodePool;
  }
  e.k_dom = e.dom_np ? e.k_nodepool : e.dom_ct ? e.k_ct : e.k_zone;
}

uint32_t Ctx::key_of(uint32_t sid) const { return e.key_id.at(label_normalize(S(sid))); }

KReq Ctx::kreq_of(const gs_requirement& q) const {
  uint32_t k = key_of(q.key);
  const Vocab& v = e.keys[k].vocab;
  std::vector<uint32_t> vals;
  int64_t bound = 0;
  if (q.op == GS_OP_IN || q.op == GS_OP_NOTIN)
    for (uint32_t i = 0; i < q.values.count; i++) vals.push_back(v.id.at(S(p->value_ids[q.values.begin + i])));
  int op = (int)q.op;
  if (op >= GS_OP_GT) go_atoi64(S(p->value_ids[q.values.begin]), &bound);
  // over integer label values Gte x is Gt x-1 and Lte x is Lt x+1
  if (op == GS_OP_GTE) {
    op = GS_OP_GT;
    bound -= 1;
  } else if (op == GS_OP_LTE) {
    op = GS_OP_LT;
    bound += 1;
  }
  KReq r = make_kreq(v, op, vals, bound);
  r.mv = q.min_values >= 0 ? q.min_values : -1;
  return r;
}
// a pod's NodeSelectorRequirement carries no minValues
void Ctx::no_min_values(gs_range r) const {
  chk(r, p->n_reqs, "reqs");
  for (uint32_t i = 0; i < r.count; i++)
    if (p->reqs[r.begin + i].min_values >= 0)
      throw Fail{GS_E_UNSUPPORTED, "minValues outside NodePool / NodeClaim requirements"};
}
Reqs Ctx::reqs_of(gs_range r) const {
  Reqs out;
  for (uint32_t i = 0; i < r.count; i++) {
    auto& q = p->reqs[r.begin + i];
    reqs_add(e, out, key_of(q.key), kreq_of(q));
  }
  return out;
}
KReq Ctx::in_one(uint32_t key, const std::string& val) const {
  const Vocab& v = e.keys[key].vocab;
  return make_kreq(v, GS_OP_IN, {v.id.at(val)}, 0);
}
KReq Ctx::in_one_or_omega(uint32_t key, const std::string& val) const {
  const Vocab& v = e.keys[key].vocab;
  auto f = v.id.find(val);
  return make_kreq(v, GS_OP_IN, {f == v.id.end() ? v.omega : f->second}, 0);
}
Reqs Ctx::node_labels_reqs(gs_range r) const {
  Reqs out;
  for (uint32_t i = 0; i < r.count; i++) {
    uint32_t k = key_of(p->labels[r.begin + i].key);
    reqs_add(e, out, k, in_one_or_omega(k, S(p->labels[r.begin + i].value)));
  }
  return out;
}
Reqs Ctx::labels_reqs(gs_range r) const {
  Reqs out;
  for (uint32_t i = 0; i < r.count; i++) {
    uint32_t k = key_of(p->labels[r.begin + i].key);
    reqs_add(e, out, k, in_one(k, S(p->labels[r.begin + i].value)));
  }
  return out;
}

}  // namespace gsh::enc
