// encode_nodes.cpp — the encoder's node phase: existing nodes in Solve order.
#include "encode_ctx.hpp"

#include <algorithm>
#include <numeric>
#include <set>

namespace gsh::enc {

// <U> ExistingNode: labels + hostname In[name]; initialized first, then name
void Ctx::build_nodes() {
  e.NN = p->n_nodes;
  std::vector<uint32_t> order(e.NN);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const bool ia = p->nodes[a].initialized != 0, ib = p->nodes[b].initialized != 0;
    if (ia != ib) return ia;
    return S(p->nodes[a].name) < S(p->nodes[b].name);
  });
  e.node_order = order;
  e.nodes.assign(e.NN, gsd::NodeRec{});
  node_taints.assign(e.NN, {});
  e.n_fk.assign((size_t)std::max<uint32_t>(e.NN, 1) * std::max<uint32_t>(e.F, 1), gsd::FK{});
  // keys some pod variant constrains with NotIn/DoesNotExist: a node lacking
  // such a non-free key would gain dynamic state there (refused below)
  std::set<uint32_t> exempt_keys;
  for (auto& pv : e.variants)
    for (auto& kv : pv.reqs)
      if (e.keys[kv.first].cls != KEY_FREE && e.keys[kv.first].shadow < 0 && exempt(kv.second))
        exempt_keys.insert(kv.first);
  for (uint32_t pos = 0; pos < e.NN; pos++) {
    const gs_node& g = p->nodes[order[pos]];
    gsd::NodeRec& nr = e.nodes[pos];
    for (int k = 0; k < gsd::KMAX_IT; k++) nr.vid[k] = gsd::NONE;
    nr.zvid = nr.cvid = gsd::NONE;
    nr.dvid = gsd::DVID_NONE;
    Reqs reqs = node_labels_reqs(g.labels);
    uint32_t hk = e.k_hostname;
    reqs_add(e, reqs, hk, in_one_or_omega(hk, S(g.name)));
    for (auto& kv : reqs) {
      const Key& key = e.keys[kv.first];
      if (key.cls == KEY_FREE) {
        e.n_fk[(size_t)pos * e.F + key.slot] = to_fk(kv.second);
        continue;
      }
      if (key.shadow >= 0) e.n_fk[(size_t)pos * e.F + key.shadow] = to_fk(kv.second);
      // a label is In[v]: exactly one has-bit
      uint32_t vid = gsd::NONE;
      for (size_t i = 0; i < key.vocab.size(); i++)
        if (kv.second.has.test(i)) vid = (uint32_t)i;
      if (key.cls == KEY_IT) nr.vid[key.slot] = vid;
      else if (key.cls == KEY_ZONE) nr.zvid = vid;
      else nr.cvid = vid;
    }
    {
      // the topology domain key's value (zone, capacity type or NodePool)
      auto fd = reqs.find(e.k_dom);
      if (fd != reqs.end())
        for (size_t i = 0; i < e.keys[e.k_dom].vocab.size(); i++)
          if (fd->second.has.test(i)) nr.dvid = (uint16_t)i;
    }
    for (uint32_t k : exempt_keys) {
      bool has = reqs.count(k) != 0;
      if (!has)
        throw Fail{GS_E_UNSUPPORTED, "existing node lacks a label that a pod constrains with NotIn/DoesNotExist (" +
                                         e.keys[k].name + ": no free slot left, or its vocabulary exceeds 255 values)"};
    }
    bool present[gsd::RMAX] = {false};
    resvec_fn(g.available, nr.avail, present);
    nr.ok = 1;
    for (uint32_t r = 0; r < e.R; r++)
      if (present[r] && nr.avail[r] < 0) nr.ok = 0;  // <U> Fits: negative total never fits
    resvec_fn(g.requests, nr.req, nullptr);
    nr.taints = 0;  // build_taint_classes
    node_taints[pos] = state_taint_ids(g);
    nr.init = g.initialized ? 1u : 0u;
  }
}

}  // namespace gsh::enc
