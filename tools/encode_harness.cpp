// encode_harness.cpp — host-only driver of the Solve encoder (encode.cpp and
// the units it drives: vocab, catalog, taints, pods, nodes, topology, reqs, par)
// and of the Create re-filter's host side (filter_encode.cpp, filter_rules.hpp)
// over gs_problem dumps written by gpusched.problem.Problem.dump().
// Built with g++ (no HIP) for three uses:
//  * sanitizers: tests/test_encode_sanitizers.py builds it with
//    -fsanitize=address,undefined and runs every dump once;
//  * profiling: build with -O2 -pg and run a dump many times (gprof);
//  * comparing encodings (two builds, two thread counts): -d prints a digest
//    of everything the encoder produced.
// Usage: encode_harness [-n reps] [-d] dump...   prints "<status> <ms> <path>"
// per dump; with -d then the message, one "<array> <length> <FNV-1a 64>" line
// per Encoded array and one "host" line over the host-only decode state.
//
// encode_harness -f catalog.gspd claims.gspd ...   (pairs) is the Create
// re-filter on the CPU: the first dump's catalog and the second dump's claim
// queries are reduced as gs_create_filter_prepare and gs_create_filter_run
// reduce them (the claims against the catalog's vocabularies, with call-local
// ids and the catalog's resource columns), laid out by the same two images,
// and pair_verdict — the rule both kernels call — is evaluated for every
// (claim, instance type) pair.  Where both paths name one file the per-call
// form of gs_create_filter (one reduction, claims first) runs too, and any
// bit the two forms disagree on makes the exit status 3.  Prints
// "<status> <catalog> <claims>" per pair and then the message of a refusal or, per claim,
// "<n_compatible> <selected> <capacity_type> <Create words> <requirements words>"
// (bitset words in hex, comma-separated, "-" for a catalog without types).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../karpenter-provider-ibm-cloud_amd/csrc/encode.hpp"
#include "../karpenter-provider-ibm-cloud_amd/csrc/filter_encode.hpp"

namespace {

struct Dump {
  std::vector<std::string> strs;
  std::vector<const char*> ptrs;
  std::vector<std::vector<char>> arrays;
  gs_problem p{};
  const gs_claim_query* queries = nullptr;
  uint32_t n_queries = 0;
};

bool read_exact(FILE* f, void* dst, size_t n) { return fread(dst, 1, n, f) == n; }

// layout: magic "GSPD", u32 version 5, u32 n_strings, per string u32 len +
// bytes, then 21 arrays in gs_problem order (value_ids .. namespaces) and the
// claim queries, each u64 count + u64 element size + raw bytes
bool load(const char* path, Dump& d) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char magic[4];
  uint32_t ver = 0, ns = 0;
  bool ok = read_exact(f, magic, 4) && memcmp(magic, "GSPD", 4) == 0 && read_exact(f, &ver, 4) && ver == 5 &&
            read_exact(f, &ns, 4);
  for (uint32_t i = 0; ok && i < ns; i++) {
    uint32_t len = 0;
    ok = read_exact(f, &len, 4);
    std::string s(len, '\0');
    ok = ok && (len == 0 || read_exact(f, &s[0], len));
    d.strs.push_back(std::move(s));
  }
  for (int a = 0; ok && a < 22; a++) {
    uint64_t n = 0, es = 0;
    ok = read_exact(f, &n, 8) && read_exact(f, &es, 8);
    std::vector<char> buf(n * es);
    ok = ok && (buf.empty() || read_exact(f, buf.data(), buf.size()));
    d.arrays.push_back(std::move(buf));
  }
  fclose(f);
  if (!ok) return false;
  for (auto& s : d.strs) d.ptrs.push_back(s.c_str());
  auto A = [&](int i) -> const void* { return d.arrays[i].empty() ? nullptr : d.arrays[i].data(); };
  auto N = [&](int i, size_t es) { return (uint32_t)(d.arrays[i].size() / es); };
  gs_problem& p = d.p;
  p.strings = d.ptrs.data();
  p.n_strings = ns;
  p.value_ids = (const uint32_t*)A(0), p.n_value_ids = N(0, 4);
  p.reqs = (const gs_requirement*)A(1), p.n_reqs = N(1, sizeof(gs_requirement));
  p.quantities = (const gs_quantity*)A(2), p.n_quantities = N(2, sizeof(gs_quantity));
  p.labels = (const gs_label*)A(3), p.n_labels = N(3, sizeof(gs_label));
  p.taints = (const gs_taint*)A(4), p.n_taints = N(4, sizeof(gs_taint));
  p.tolerations = (const gs_toleration*)A(5), p.n_tolerations = N(5, sizeof(gs_toleration));
  p.terms = (const gs_term*)A(6), p.n_terms = N(6, sizeof(gs_term));
  p.it_refs = (const uint32_t*)A(7), p.n_it_refs = N(7, 4);
  p.offerings = (const gs_offering*)A(8), p.n_offerings = N(8, sizeof(gs_offering));
  p.instance_types = (const gs_instance_type*)A(9), p.n_instance_types = N(9, sizeof(gs_instance_type));
  p.nodepools = (const gs_nodepool*)A(10), p.n_nodepools = N(10, sizeof(gs_nodepool));
  p.pods = (const gs_pod*)A(11), p.n_pods = N(11, sizeof(gs_pod));
  p.nodes = (const gs_node*)A(12), p.n_nodes = N(12, sizeof(gs_node));
  p.spreads = (const gs_spread*)A(13), p.n_spreads = N(13, sizeof(gs_spread));
  p.bound_pods = (const gs_pod*)A(14), p.n_bound_pods = N(14, sizeof(gs_pod));
  p.bound_pod_node = (const uint32_t*)A(15);
  p.affinity_terms = (const gs_affinity_term*)A(16), p.n_affinity_terms = N(16, sizeof(gs_affinity_term));
  p.host_ports = (const gs_host_port*)A(17), p.n_host_ports = N(17, sizeof(gs_host_port));
  p.volumes = (const gs_volume*)A(18), p.n_volumes = N(18, sizeof(gs_volume));
  p.volume_limits = (const gs_volume_limit*)A(19), p.n_volume_limits = N(19, sizeof(gs_volume_limit));
  p.namespaces = (const gs_namespace*)A(20), p.n_namespaces = N(20, sizeof(gs_namespace));
  d.queries = (const gs_claim_query*)A(21), d.n_queries = N(21, sizeof(gs_claim_query));
  return true;
}

// 64-bit FNV-1a
struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void* p, size_t n) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  }
  void str(const std::string& s) {
    u64(s.size());
    bytes(s.data(), s.size());
  }
  void u64(uint64_t x) { bytes(&x, 8); }
};

template <class T>
void digest_array(const char* name, const std::vector<T>& v) {
  Fnv f;
  f.bytes(v.data(), v.size() * sizeof(T));
  printf("  %s %zu %016llx\n", name, v.size(), (unsigned long long)f.h);
}

void digest(const gsh::Err& er, const gsh::Encoded& e) {
  printf("  msg %s\n", er.msg.c_str());
#define A(m) digest_array(#m, e.m)
  A(it_keys), A(free_keys), A(cat_zone), A(cat_ct), A(res_name_ids);
  A(it_vid), A(it_prank), A(it_namerank), A(rank_to_it), A(thr_off), A(it_dvid), A(it_ndv);
  A(n_vol), A(pod_vol), A(pod_vfresh);
  A(it_alloc), A(it_cap), A(thr_val), A(fk_ival), A(it_pair), A(slot_set), A(thr_set), A(fk_isint);
  A(prices), A(t_limopts), A(tmpl), A(t_opts), A(t_fk), A(pod_req), A(var_begin), A(var_count), A(queue0);
  A(var_sv), A(vars), A(itmask), A(var_itclass), A(itclass_mask), A(fk_entries);
  A(node_order), A(nodes), A(n_fk);
  A(tgroups), A(tg_list), A(zcnt0), A(htot0), A(lazy_slot), A(var_lz_off), A(lz_idx), A(lz_mind);
  A(zone_order), A(zone_cat), A(hn0), A(zn_cnt), A(zone_nodes);
#undef A
  // host-only state: vocabulary, sizes and flags, then the requirement sets decode reads
  Fnv f;
  for (auto& k : e.keys) {
    f.str(k.name);
    for (auto& v : k.vocab.vals) f.str(v);
    f.u64(((uint64_t)k.cls << 40) | ((uint64_t)k.wellknown << 32) | (uint32_t)k.slot);
    f.u64((uint32_t)k.shadow);
  }
  for (auto& r : e.res_names) f.str(r);
  for (uint64_t x : {(uint64_t)e.k_zone, (uint64_t)e.k_ct, (uint64_t)e.k_hostname, (uint64_t)e.k_nodepool, (uint64_t)e.k_dom,
                     (uint64_t)e.dom_ct, (uint64_t)e.dom_np, (uint64_t)e.N, (uint64_t)e.W, (uint64_t)e.R, (uint64_t)e.Z,
                     (uint64_t)e.C, (uint64_t)e.T, (uint64_t)e.F, (uint64_t)e.V, (uint64_t)e.P, (uint64_t)e.K,
                     (uint64_t)e.NT, e.wk_slots, e.checks, e.checks_per_pod, (uint64_t)e.it_key_unique,
                     (uint64_t)e.any_mv, (uint64_t)e.any_vol, (uint64_t)e.NN, (uint64_t)e.TG, (uint64_t)e.TGH,
                     (uint64_t)e.TGZ, (uint64_t)e.NZV, (uint64_t)e.ZS, (uint64_t)e.n_lazy, e.known_np, e.zknown0})
    f.u64(x);
  for (auto& r : e.tmpl_reqs) f.str(gsh::canonical(e, r));
  for (auto& v : e.variants) {
    f.str(gsh::canonical(e, v.reqs));
    f.str(gsh::canonical(e, v.strict));
    f.u64(v.tol);
    f.u64(v.own.size());
    for (uint32_t g : v.own) f.u64(g);
    f.u64(v.lazy_mind.size());
    for (auto& lm : v.lazy_mind) f.u64(((uint64_t)lm.first << 32) | (uint32_t)lm.second);
  }
  printf("  host %zu %zu %016llx\n", e.tmpl_reqs.size(), e.variants.size(), (unsigned long long)f.h);
}

// ------------------------------------------------ the Create re-filter (-f)
using namespace gsf;

// what DevSelect is on the device: the catalog's image and the claims' image
// under host addresses.  Dense value ids below V are the catalog's.
struct HostView {
  const FReq* reqs;
  const uint32_t* vals;
  const int64_t* vint;
  const uint8_t* vok;
  const FIt* its;
  const FOff* offs;
  const int64_t* alloc;
  uint32_t N, R, V;
  const FReq* q_reqs;
  const uint32_t* q_vals;
  const int64_t* q_vint;
  const uint8_t* q_vok;
  const FQuery* qs;
  const FQty* qty;
  bool vok_at(uint32_t v) const { return v < V ? vok[v] : q_vok[v - V]; }
  int64_t vint_at(uint32_t v) const { return v < V ? vint[v] : q_vint[v - V]; }
};

struct Verdicts {
  gs_status status = GS_OK;
  std::string msg;
  uint32_t W = 0;
  std::vector<uint64_t> create, reqs, spot;  // [Q][W]
  std::vector<uint32_t> n, ct;
  std::vector<int32_t> sel;
  bool operator==(const Verdicts& o) const {
    return status == o.status && W == o.W && create == o.create && reqs == o.reqs && spot == o.spot && n == o.n &&
           ct == o.ct && sel == o.sel;
  }
};

// pair_verdict over every pair, folded as the kernels and their callers fold it
void evaluate(const HostView& d, uint32_t nq, Verdicts& out) {
  const uint32_t W = (d.N + 63) / 64;
  out.W = W;
  out.create.assign((size_t)nq * W, 0);
  out.reqs.assign((size_t)nq * W, 0);
  out.spot.assign((size_t)nq * W, 0);
  out.n.assign(nq, 0);
  out.sel.assign(nq, -1);
  out.ct.assign(nq, GS_CAPACITY_ON_DEMAND);
  for (uint32_t q = 0; q < nq; q++) {
    const FQuery Q = d.qs[q];
    bool spot = false;
    for (uint32_t it = 0; it < d.N; it++) {
      const uint32_t ok = pair_verdict(d, Q, d.q_reqs + Q.reqs.b, d.q_vals, d.reqs, d.vals, it);
      const size_t w = (size_t)q * W + (it >> 6);
      const uint64_t bit = 1ull << (it & 63);
      if (ok & P_REQS) out.reqs[w] |= bit;
      if (ok & P_CREATE) {
        out.create[w] |= bit;
        if (out.sel[q] < 0) out.sel[q] = (int32_t)it;
        out.n[q]++;
      }
      if (ok & P_SPOT) out.spot[w] |= bit, spot = true;
    }
    if (Q.spot && spot) out.ct[q] = GS_CAPACITY_SPOT;
  }
}

// gs_create_filter_prepare on cat, then gs_create_filter_run of pool's claims
Verdicts filter_prepared(const gs_problem* cat, const gs_problem* pool, const gs_claim_query* qs, uint32_t nq) {
  Verdicts out;
  if (null_with_count(cat, true) || null_with_count(pool, false)) {
    out.status = GS_E_INVALID;
    return out;
  }
  try {
    Enc ce;
    ce.p = cat;
    Columns cc;
    std::vector<FIt> its;
    std::vector<FOff> offs;
    std::vector<int64_t> alloc;
    capacity_columns(ce, cc);
    encode_catalog(ce, cc.id, cc.R, its, offs, alloc, nullptr);
    Image ci;
    const CatalogImage cimg(ci, ce, its, offs, alloc);
    std::vector<char> hc(ci.off);
    cimg.fill(hc.data(), ce, its, offs, alloc);
    // ids for this call only, above the catalog's
    Enc e;
    e.p = pool;
    e.base = &ce;
    e.kb = (uint32_t)ce.key_name.size();
    e.vb = (uint32_t)ce.vint.size();
    Columns cols;
    cols.catalog = &cc;
    std::vector<FQuery> fq;
    std::vector<FQty> qty;
    encode_claims(e, qs, nq, resident_column, cols, fq, qty);
    Image qi;
    const ClaimImage qimg(qi, &e, fq, qty);
    std::vector<char> hq(qi.off);
    qimg.fill(hq.data(), &e, fq, qty);
    HostView d{};
    cimg.bind(hc.data(), d);
    qimg.bind(hq.data(), d);
    qimg.bind_lists(hq.data(), d);
    d.N = cat->n_instance_types;
    d.R = cc.R;
    d.V = e.vb;
    evaluate(d, nq, out);
  } catch (const Fail& f) {
    out.status = f.code;
    out.msg = f.msg;
  }
  return out;
}

// gs_create_filter: one reduction (claims first), one arena
Verdicts filter_per_call(const gs_problem* p, const gs_claim_query* qs, uint32_t nq) {
  Verdicts out;
  if (null_with_count(p, true)) {
    out.status = GS_E_INVALID;
    return out;
  }
  try {
    Enc e;
    e.p = p;
    Columns cols;
    std::vector<FIt> its;
    std::vector<FOff> offs;
    std::vector<FQuery> fq;
    std::vector<FQty> qty;
    std::vector<int64_t> alloc;
    encode_claims(e, qs, nq, call_column, cols, fq, qty);
    const uint32_t R = std::max<uint32_t>(1, (uint32_t)cols.id.size());
    encode_catalog(e, cols.id, R, its, offs, alloc, nullptr);
    Image im;
    const CatalogImage cat(im, e, its, offs, alloc);
    const ClaimImage claims(im, nullptr, fq, qty);
    std::vector<char> h(im.off);
    cat.fill(h.data(), e, its, offs, alloc);
    claims.fill(h.data(), nullptr, fq, qty);
    HostView d{};
    cat.bind(h.data(), d);
    claims.bind(h.data(), d);
    d.q_reqs = d.reqs;  // one Enc: the claims' lists and values are the catalog image's
    d.q_vals = d.vals;
    d.N = p->n_instance_types;
    d.R = R;
    d.V = ~0u;
    evaluate(d, nq, out);
  } catch (const Fail& f) {
    out.status = f.code;
    out.msg = f.msg;
  }
  return out;
}

void print_words(const uint64_t* w, uint32_t n) {
  if (!n) printf("-");
  for (uint32_t i = 0; i < n; i++) printf("%s%llx", i ? "," : "", (unsigned long long)w[i]);
}

int filter_main(int argc, char** argv, int i) {
  int rc = 0;
  for (; i + 1 < argc; i += 2) {
    Dump cat, claims;
    if (!load(argv[i], cat) || !load(argv[i + 1], claims)) {
      fprintf(stderr, "cannot read %s or %s\n", argv[i], argv[i + 1]);
      rc = 2;
      continue;
    }
    const Verdicts v = filter_prepared(&cat.p, &claims.p, claims.queries, claims.n_queries);
    if (strcmp(argv[i], argv[i + 1]) == 0 && !(filter_per_call(&cat.p, cat.queries, cat.n_queries) == v)) {
      fprintf(stderr, "%s: the per-call and the prepared form disagree\n", argv[i]);
      rc = 3;
    }
    printf("%d %s %s\n", (int)v.status, argv[i], argv[i + 1]);
    if (v.status != GS_OK) {
      printf("  msg %s\n", v.msg.c_str());
      continue;
    }
    for (uint32_t q = 0; q < claims.n_queries; q++) {
      printf("%u %d %u ", v.n[q], v.sel[q], v.ct[q]);
      print_words(v.create.data() + (size_t)q * v.W, v.W);
      printf(" ");
      print_words(v.reqs.data() + (size_t)q * v.W, v.W);
      printf("\n");
    }
  }
  if (i < argc) {
    fprintf(stderr, "-f takes pairs of dumps\n");
    rc = 2;
  }
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  int reps = 1, i = 1;
  bool dump = false;
  for (; i < argc && argv[i][0] == '-'; i++) {
    if (strcmp(argv[i], "-f") == 0) return filter_main(argc, argv, i + 1);
    if (strcmp(argv[i], "-d") == 0) dump = true;
    else if (strcmp(argv[i], "-n") == 0 && i + 1 < argc) reps = atoi(argv[++i]);
    else break;
  }
  int rc = 0;
  for (; i < argc; i++) {
    Dump d;
    if (!load(argv[i], d)) {
      fprintf(stderr, "cannot read %s\n", argv[i]);
      rc = 2;
      continue;
    }
    gsh::Err er;
    double best = 1e300;
    gsh::Encoded e;  // one per dump, reused across reps (as a context reuses its encoding)
    for (int r = 0; r < reps; r++) {
      auto t0 = std::chrono::steady_clock::now();
      er = gsh::encode(&d.p, e);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (ms < best) best = ms;
    }
    printf("%d %.3f %s\n", (int)er.code, best, argv[i]);
    if (dump) digest(er, e);
  }
  return rc;
}
