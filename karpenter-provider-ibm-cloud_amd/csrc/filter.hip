// filter.hip — launch-time re-filter of emitted NodeClaims (gs_create_filter
// and its prepared form gs_create_filter_prepare / _run / _set_available):
// CloudProvider.Create's instance-type filter (reference
// pkg/cloudprovider/cloudprovider.go:322-346), GetInstanceTypes' NodePool
// filter (:574-577), the instance provider's instanceTypes[0] pick
// (pkg/providers/vpc/instance/provider.go:215-221) and ResolveCapacityType
// (pkg/providers/common/capacitytype/capacitytype.go:27-42), for a batch of
// NodeClaims in one device pass.
//
// This unit holds the two kernels, the state and the entry points.  The
// records and the rule for one (claim, instance type) pair are in
// filter_rules.hpp; the host reduction of the caller's requirement lists and
// the two images are in filter_encode.hpp / filter_encode.cpp (host only, and
// run on the CPU under sanitizers by tests/test_encode_sanitizers.py).
//
// HBM layout (gs_create_filter: one arena per call):
//   reqs[]  FReq (32 B) — all requirement lists, key-sorted within a list
//   vals[]  u32 dense value ids, sorted within a requirement
//   vint[]  i64 parsed value (strconv.Atoi) per dense value, vok[] u8 parse ok
//   its[]   FIt: requirement list, offering range, Allocatable() < 0 flag
//   offs[]  FOff: requirement list, Available, Requirements.Get(ct).Has(spot)
//   alloc[] i64 [N][R]: Allocatable() over the resources the claims request
//   qs[]    FQuery: requirement list + request range into qty[]
//   out     u64 bitsets [Q][W] x3 (Create filter, requirements-only, spot)
//
// The prepared form splits the arena in two.  The catalog part (CatalogImage:
// reqs, vals, vint, vok, its, offs, alloc over every resource a capacity list
// names) stays on the device from gs_create_filter_prepare on; a run uploads
// only the claims' part (ClaimImage: their reqs, vals, the vint / vok of
// values the catalog does not know, qs, qty) and reads back one 16-B record
// per claim, plus the Create and requirements bitsets under GS_CF_BITSETS.
// Keys and values the catalog knows keep the ids the prepare gave them; the
// others get ids above the catalog's for the one call.
#include "ctx.hpp"
#include "filter_encode.hpp"

namespace gsf {

struct DevFilter {
  const FReq* reqs;
  const uint32_t* vals;
  const int64_t* vint;
  const uint8_t* vok;
  const FIt* its;
  const FOff* offs;
  const int64_t* alloc;
  const FQuery* qs;
  const FQty* qty;
  uint32_t N, Q, R, W;
  uint64_t* out_create;
  uint64_t* out_reqs;
  uint64_t* out_spot;
  __device__ bool vok_at(uint32_t v) const { return vok[v]; }
  __device__ int64_t vint_at(uint32_t v) const { return vint[v]; }
};

// The prepared form's two halves.  Dense value ids below V are the resident
// catalog's (vint / vok), the others the call's (q_vint / q_vok at id - V);
// a requirement's vb indexes the vals array of the half it came from.
struct DevSelect {
  const FReq* reqs;
  const uint32_t* vals;
  const int64_t* vint;
  const uint8_t* vok;
  const FIt* its;
  const FOff* offs;
  const int64_t* alloc;
  uint32_t N, R, W, V;
  const FReq* q_reqs;
  const uint32_t* q_vals;
  const int64_t* q_vint;
  const uint8_t* q_vok;
  const FQuery* qs;
  const FQty* qty;
  FRec* out_rec;
  uint64_t* out_create;  // nullptr without GS_CF_BITSETS
  uint64_t* out_reqs;
  __device__ bool vok_at(uint32_t v) const { return v < V ? vok[v] : q_vok[v - V]; }
  __device__ int64_t vint_at(uint32_t v) const { return v < V ? vint[v] : q_vint[v - V]; }
};

// ----------------------------------------------------------------- device
// one lane per (claim, instance type); blockIdx.y = claim, 256 types per block
__global__ __launch_bounds__(256) void claim_filter_kernel(DevFilter d) {
  const uint32_t q = blockIdx.y;
  const uint32_t it = blockIdx.x * 256 + threadIdx.x;
  uint32_t ok = 0;
  if (it < d.N) {
    const FQuery Q = d.qs[q];
    ok = pair_verdict(d, Q, d.reqs + Q.reqs.b, d.vals, d.reqs, d.vals, it);
  }
  const uint64_t b_req = __ballot(ok & P_REQS), b_create = __ballot(ok & P_CREATE), b_spot = __ballot(ok & P_SPOT);
  const uint32_t w = it >> 6;
  if ((threadIdx.x & 63) == 0 && w < d.W) {
    const size_t o = (size_t)q * d.W + w;
    d.out_reqs[o] = b_req;
    d.out_create[o] = b_create;
    d.out_spot[o] = b_spot;
  }
}

// The prepared form: one 256-thread workgroup per claim (blockIdx.x), looping
// over the instance types 256 at a time, one lane per pair.  The claim's list
// is staged in LDS when it fits sel_fits_lds (a per-workgroup choice, so the
// barrier after it is reached by every thread) and read from HBM otherwise.
// Per chunk the three wave ballots are the bitset words (stored only when the
// caller asked for bitsets); each wave keeps the Create ballot's population
// count, its lowest set index and whether a spot bit was set, the four waves
// meet in LDS, and thread 0 stores the claim's FRec.
__global__ __launch_bounds__(256) void claim_select_kernel(DevSelect d) {
  __shared__ FReq s_reqs[kSelLdsReqs];
  __shared__ uint32_t s_vals[kSelLdsVals];
  __shared__ uint32_t s_cnt[4], s_first[4], s_spot[4];
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const FQuery Q = d.qs[q];
  const bool staged = sel_fits_lds(Q.reqs.n, Q.vn);
  if (staged) {
    for (uint32_t i = t; i < Q.reqs.n; i += 256) {
      FReq r = d.q_reqs[Q.reqs.b + i];
      r.vb -= Q.vb;  // into s_vals
      s_reqs[i] = r;
    }
    for (uint32_t i = t; i < Q.vn; i += 256) s_vals[i] = d.q_vals[Q.vb + i];
  }
  __syncthreads();
  const FReq* qr = staged ? s_reqs : d.q_reqs + Q.reqs.b;
  const uint32_t* qv = staged ? s_vals : d.q_vals;
  uint32_t cnt = 0, first = ~0u, spot = 0;  // wave-uniform: they follow the ballots
  for (uint32_t base = 0; base < d.N; base += 256) {
    const uint32_t it = base + t;
    const uint32_t ok = it < d.N ? pair_verdict(d, Q, qr, qv, d.reqs, d.vals, it) : 0;
    const uint64_t b_req = __ballot(ok & P_REQS), b_create = __ballot(ok & P_CREATE), b_spot = __ballot(ok & P_SPOT);
    const uint32_t w = it >> 6;
    if (d.out_create && (t & 63) == 0 && w < d.W) {
      const size_t o = (size_t)q * d.W + w;
      d.out_reqs[o] = b_req;
      d.out_create[o] = b_create;
    }
    if (b_create && first == ~0u) first = (it & ~63u) + (uint32_t)__builtin_ctzll(b_create);
    cnt += (uint32_t)__builtin_popcountll(b_create);
    spot |= b_spot != 0;
  }
  if ((t & 63) == 0) {
    s_cnt[t >> 6] = cnt;
    s_first[t >> 6] = first;
    s_spot[t >> 6] = spot;
  }
  __syncthreads();
  if (t == 0) {
    FRec r{};
    uint32_t f = ~0u, sp = 0;
    for (uint32_t w = 0; w < 4; w++) {
      r.n_compatible += s_cnt[w];
      f = s_first[w] < f ? s_first[w] : f;
      sp |= s_spot[w];
    }
    r.selected = (int32_t)f;  // ~0u: -1
    r.capacity_type = (Q.spot && sp) ? GS_CAPACITY_SPOT : GS_CAPACITY_ON_DEMAND;
    d.out_rec[q] = r;
  }
}

// ------------------------------------------------------------------ state
// gs_create_filter_prepare's catalog, resident on the device, and the
// buffers and results of the runs against it
struct Resident {
  bool ready = false;
  Enc voc;       // the catalog's key and value vocabularies (no lists)
  Columns cols;  // alloc[] columns: every resource a capacity list names
  uint32_t N = 0, W = 0;
  std::vector<FOff> offs;                    // host mirror of the device array
  std::vector<std::vector<uint32_t>> slots;  // catalog offering index -> positions in offs
  gsc::DevBuf cat_dev;                       // the catalog image
  CatalogImage cat;
  // a run's claim image and outputs: grow-once device arena, pinned host sides
  gsc::DevBuf run_dev;
  gsc::PinnedBuf h_in, h_out;
  std::vector<uint32_t> res_n, res_ct;
  std::vector<int32_t> res_sel;
  gs_create_filter_stats stats{};
};

// everything the re-filter keeps in a context (gs_ctx::cf, made on first use)
struct State {
  // gs_create_filter: grow-once device arena and result storage
  gsc::DevBuf dev;
  std::vector<uint64_t> create, reqs, spot;
  std::vector<uint32_t> n, ct;
  std::vector<int32_t> sel;
  // gs_create_filter_prepare / _run: separate from the arena above
  Resident res;
};

}  // namespace gsf

using namespace gsc;
using namespace gsf;

static State& state(gs_ctx* c) {
  if (!c->cf) c->cf = new State;
  return *c->cf;
}

void gsc::create_filter_destroy(gs_ctx* c) {
  delete c->cf;  // its buffers with it
  c->cf = nullptr;
}

extern "C" gs_status gs_create_filter(gs_ctx* c, const gs_problem* p, const gs_claim_query* qs, uint32_t nq,
                                      gs_claim_filter_result* out) {
  if (!c || !p || !out || (nq && !qs)) return GS_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  // reject before any allocation: the grid's y dimension, and every array the
  // host pass reads that is null while its count is not
  if (nq > 65535u) return fail(c, GS_E_INVALID, "more than 65535 claims in one gs_create_filter call");
  if (null_with_count(p, true)) return fail(c, GS_E_INVALID, "null array with a non-zero count");
  Enc e;
  e.p = p;
  std::vector<FIt> its;
  std::vector<FOff> offs;
  std::vector<FQuery> fq;
  std::vector<FQty> qty;
  std::vector<int64_t> alloc;
  uint32_t R = 0;
  const uint32_t N = p->n_instance_types;
  try {
    // claims first: their requested resources form the Fits vocabulary
    Columns cols;
    encode_claims(e, qs, nq, call_column, cols, fq, qty);
    R = std::max<uint32_t>(1, (uint32_t)cols.id.size());
    encode_catalog(e, cols.id, R, its, offs, alloc, nullptr);
  } catch (const Fail& f) {
    return fail(c, f.code, f.msg);
  }
  State& s = state(c);
  const uint32_t W = (N + 63) / 64;
  s.create.assign((size_t)nq * W, 0);
  s.reqs.assign((size_t)nq * W, 0);
  s.spot.assign((size_t)nq * W, 0);
  if (nq && N) {
    try {
      HIPCHK(hipSetDevice(c->device));
      // one arena: inputs then the three output bitsets
      Image im;
      const CatalogImage cat(im, e, its, offs, alloc);
      const ClaimImage claims(im, nullptr, fq, qty);
      const size_t o_out = im.place((size_t)3 * nq * W * 8);
      s.dev.reserve_exact(im.off);
      char* base = (char*)s.dev.data();
      // staging: one host copy, one H2D transfer
      std::vector<char> h(o_out);
      cat.fill(h.data(), e, its, offs, alloc);
      claims.fill(h.data(), nullptr, fq, qty);
      HIPCHK(hipMemcpyAsync(base, h.data(), o_out, hipMemcpyHostToDevice, c->stream));
      DevFilter d{};
      cat.bind(base, d);
      claims.bind(base, d);
      d.N = N;
      d.Q = nq;
      d.R = R;
      d.W = W;
      d.out_create = (uint64_t*)(base + o_out);
      d.out_reqs = d.out_create + (size_t)nq * W;
      d.out_spot = d.out_reqs + (size_t)nq * W;
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      hipLaunchKernelGGL(claim_filter_kernel, dim3((N + 255) / 256, nq), dim3(256), 0, c->stream, d);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      const size_t ob = (size_t)nq * W * 8;
      HIPCHK(hipMemcpyAsync(s.create.data(), d.out_create, ob, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(s.reqs.data(), d.out_reqs, ob, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(s.spot.data(), d.out_spot, ob, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      // nothing reads this time.  The two records and the query stay because a
      // call measured 6 to 10 us slower without them (of 0.93 ms on CM's
      // claims; profiles/r8/create_filter_split.json, "event_sequence")
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    } catch (const HipError& ex) {
      return fail(c, GS_E_HIP, ex.msg);
    }
  }
  s.n.assign(nq, 0);
  s.sel.assign(nq, -1);
  s.ct.assign(nq, GS_CAPACITY_ON_DEMAND);
  for (uint32_t q = 0; q < nq; q++) {
    bool spot = false;
    for (uint32_t w = 0; w < W; w++) {
      const uint64_t x = s.create[(size_t)q * W + w];
      if (x && s.sel[q] < 0) s.sel[q] = (int32_t)(64 * w + __builtin_ctzll(x));
      s.n[q] += (uint32_t)__builtin_popcountll(x);
      spot |= s.spot[(size_t)q * W + w] != 0;
    }
    if (fq[q].spot && spot) s.ct[q] = GS_CAPACITY_SPOT;
  }
  out->n_queries = nq;
  out->words = W;
  out->compatible = s.create.data();
  out->requirements = s.reqs.data();
  out->n_compatible = s.n.data();
  out->selected = s.sel.data();
  out->capacity_type = s.ct.data();
  return GS_OK;
}

// ------------------------------------------------------- the prepared form
extern "C" uint32_t gs_create_filter_stats_size(void) { return (uint32_t)sizeof(gs_create_filter_stats); }

extern "C" gs_status gs_create_filter_last_run(const gs_ctx* c, gs_create_filter_stats* out) {
  if (!c || !out) return GS_E_INVALID;
  *out = c->cf ? c->cf->res.stats : gs_create_filter_stats{};
  return GS_OK;
}

extern "C" gs_status gs_create_filter_prepare(gs_ctx* c, const gs_problem* p) {
  if (!c || !p) return GS_E_INVALID;
  if (null_with_count(p, true)) return fail(c, GS_E_INVALID, "null array with a non-zero count");
  // the host encoding first: a failure leaves the resident catalog as it was
  const auto t0 = Clock::now();
  Enc e;
  e.p = p;
  Columns cols;
  std::vector<FIt> its;
  std::vector<FOff> offs;
  std::vector<int64_t> alloc;
  std::vector<std::vector<uint32_t>> slots(p->n_offerings);
  const uint32_t N = p->n_instance_types;
  try {
    capacity_columns(e, cols);
    encode_catalog(e, cols.id, cols.R, its, offs, alloc, &slots);
  } catch (const Fail& f) {
    return fail(c, f.code, f.msg);
  }
  Image im;
  const CatalogImage cat(im, e, its, offs, alloc);
  std::vector<char> h(im.off);
  cat.fill(h.data(), e, its, offs, alloc);
  const double encode_ms = ms_since(t0);
  const auto t1 = Clock::now();
  DevBuf dev;  // the new image: freed by scope on a failure
  try {
    HIPCHK(hipSetDevice(c->device));
    dev.reserve_exact(im.off);
    HIPCHK(hipMemcpyAsync(dev.data(), h.data(), im.off, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // also: no run of the old catalog is in flight
  } catch (const HipError& ex) {
    return fail(c, GS_E_HIP, ex.msg);
  }
  Resident& r = state(c).res;
  r.cat_dev = std::move(dev);  // frees the old image
  // keep the vocabularies; the lists live on the device now
  e.p = nullptr;
  e.reqs = {};
  e.vals = {};
  e.key_of = {};
  e.val_of = {};
  r.voc = std::move(e);
  r.cols = std::move(cols);
  r.N = N;
  r.W = (N + 63) / 64;
  r.offs = std::move(offs);
  r.slots = std::move(slots);
  r.cat = cat;
  r.ready = true;
  r.stats = gs_create_filter_stats{};
  r.stats.encode_ms = encode_ms;
  r.stats.upload_ms = ms_since(t1);
  r.stats.h2d_bytes = im.off;
  r.stats.n_instance_types = N;
  return GS_OK;
}

extern "C" gs_status gs_create_filter_set_available(gs_ctx* c, const uint32_t* offering, const uint8_t* available,
                                                    uint32_t n) {
  if (!c || (n && (!offering || !available))) return GS_E_INVALID;
  Resident* r = c->cf ? &c->cf->res : nullptr;
  if (!r || !r->ready)
    return fail(c, GS_E_INVALID, "gs_create_filter_set_available before gs_create_filter_prepare");
  for (uint32_t i = 0; i < n; i++)
    if (offering[i] >= r->slots.size()) return fail(c, GS_E_INVALID, "offering index out of range");
  if (!n) return GS_OK;
  for (uint32_t i = 0; i < n; i++)  // in order: a repeated index takes its last value
    for (uint32_t s : r->slots[offering[i]]) r->offs[s].available = available[i] ? 1 : 0;
  if (r->offs.empty()) return GS_OK;
  try {
    HIPCHK(hipSetDevice(c->device));
    // the whole FOff array (16 B per offering) from the patched mirror: one
    // transfer whatever n is, on the stream the next run is launched on
    HIPCHK(hipMemcpyAsync((char*)r->cat_dev.data() + r->cat.offs, r->offs.data(), r->offs.size() * sizeof(FOff),
                          hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // the mirror may change again after this call
  } catch (const HipError& ex) {
    return fail(c, GS_E_HIP, ex.msg);
  }
  return GS_OK;
}

extern "C" gs_status gs_create_filter_run(gs_ctx* c, const gs_problem* p, const gs_claim_query* qs, uint32_t nq,
                                          uint32_t flags, gs_claim_filter_result* out) {
  if (!c || !p || !out || (nq && !qs)) return GS_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (!c->cf || !c->cf->res.ready) return fail(c, GS_E_INVALID, "gs_create_filter_run before gs_create_filter_prepare");
  Resident& r = c->cf->res;
  if (flags & ~GS_CF_BITSETS) return fail(c, GS_E_INVALID, "unknown gs_create_filter_run flag");
  if (nq > 65535u) return fail(c, GS_E_INVALID, "more than 65535 claims in one gs_create_filter_run call");
  if (null_with_count(p, false)) return fail(c, GS_E_INVALID, "null array with a non-zero count");
  const auto t0 = Clock::now();
  // ids for this call only: e goes when the call returns
  Enc e;
  e.p = p;
  e.base = &r.voc;
  e.kb = (uint32_t)r.voc.key_name.size();
  e.vb = (uint32_t)r.voc.vint.size();
  std::vector<FQuery> fq;
  std::vector<FQty> qty;
  try {
    Columns cols;
    cols.catalog = &r.cols;
    encode_claims(e, qs, nq, resident_column, cols, fq, qty);
  } catch (const Fail& f) {
    return fail(c, f.code, f.msg);
  }
  uint32_t n_staged = 0;
  for (const FQuery& x : fq) n_staged += sel_fits_lds(x.reqs.n, x.vn) ? 1 : 0;
  const bool bits = flags & GS_CF_BITSETS;
  const uint32_t W = r.W;
  gs_create_filter_stats st{};
  st.n_queries = nq;
  st.n_instance_types = r.N;
  st.n_staged_lds = n_staged;
  r.res_n.assign(nq, 0);
  r.res_sel.assign(nq, -1);
  r.res_ct.assign(nq, GS_CAPACITY_ON_DEMAND);
  const uint64_t* h_create = nullptr;
  const uint64_t* h_reqs = nullptr;
  if (nq) {
    try {
      HIPCHK(hipSetDevice(c->device));
      // the claims' image, then the outputs: records, and the two bitsets when asked for
      Image im;
      const ClaimImage claims(im, &e, fq, qty);
      const size_t in_bytes = im.off;
      const size_t bs_bytes = bits ? (size_t)nq * W * 8 : 0;
      const size_t out_bytes = (size_t)nq * sizeof(FRec) + 2 * bs_bytes;
      r.run_dev.reserve(in_bytes + out_bytes);
      r.h_in.reserve(in_bytes);
      r.h_out.reserve(out_bytes);
      claims.fill((char*)r.h_in.data(), &e, fq, qty);
      st.encode_ms = ms_since(t0);
      const auto t1 = Clock::now();
      char* base = (char*)r.run_dev.data();
      HIPCHK(hipMemcpyAsync(base, r.h_in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
      st.h2d_bytes = in_bytes;
      DevSelect d{};
      r.cat.bind((const char*)r.cat_dev.data(), d);
      claims.bind(base, d);
      claims.bind_lists(base, d);
      d.N = r.N;
      d.R = r.cols.R;
      d.W = W;
      d.V = e.vb;
      d.out_rec = (FRec*)(base + in_bytes);
      if (bits) {
        d.out_create = (uint64_t*)(base + in_bytes + (size_t)nq * sizeof(FRec));
        d.out_reqs = d.out_create + (size_t)nq * W;
      }
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      hipLaunchKernelGGL(claim_select_kernel, dim3(nq), dim3(256), 0, c->stream, d);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      st.n_launches = 1;
      st.upload_ms = ms_since(t1);
      const auto t2 = Clock::now();
      HIPCHK(hipMemcpyAsync(r.h_out.data(), base + in_bytes, out_bytes, hipMemcpyDeviceToHost, c->stream));
      st.d2h_bytes = out_bytes;
      HIPCHK(hipStreamSynchronize(c->stream));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
      st.kernel_ms = ms;
      const FRec* rec = (const FRec*)r.h_out.data();
      for (uint32_t q = 0; q < nq; q++) {
        r.res_n[q] = rec[q].n_compatible;
        r.res_sel[q] = rec[q].selected;
        r.res_ct[q] = rec[q].capacity_type;
      }
      if (bits) {
        h_create = (const uint64_t*)((const char*)r.h_out.data() + (size_t)nq * sizeof(FRec));
        h_reqs = h_create + (size_t)nq * W;
      }
      st.fetch_ms = ms_since(t2);
    } catch (const HipError& ex) {
      return fail(c, GS_E_HIP, ex.msg);
    }
  } else {
    st.encode_ms = ms_since(t0);
  }
  r.stats = st;
  out->n_queries = nq;
  out->words = W;
  out->compatible = h_create;
  out->requirements = h_reqs;
  out->n_compatible = r.res_n.data();
  out->selected = r.res_sel.data();
  out->capacity_type = r.res_ct.data();
  return GS_OK;
}
