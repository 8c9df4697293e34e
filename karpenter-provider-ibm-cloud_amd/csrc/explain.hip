// explain.hip — gs_explain: why each NodePool could not take a pod
// (include/gpusched.h).  A side path of the prepared problem: its own two
// kernels and its own buffers; it reads what gs_prepare left resident and
// writes none of the Solve's or the static matrix's buffers.
//
//  explain_cursor_kernel  the Fits threshold cursors of the requested
//                         variants (feas_cursor_kernel's rule, own buffer)
//  explain_kernel         per (variant, template) pair the seven booleans of
//                         <U> filterInstanceTypesByRequirements over the
//                         template's options, the pre-checks of
//                         NodeClaim.CanAdd and the minValues verdict, folded
//                         by explain_rules.hpp into one packed word
//
// (a .hip unit: the host side needs the HIP runtime)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctx.hpp"
#include "devutil.hpp"
#include "explain_rules.hpp"

using namespace gsd;

namespace gse {

constexpr int BLOCK = 256;
constexpr uint32_t TCLS_MAX = 64;   // taint classes (encode_taints.cpp refuses more)
constexpr uint8_t TCLS_END = 0xFF;

struct ExplainArgs {
  const uint32_t* ev;   // [nv] the device variants to judge
  const uint64_t* inc;  // [nv] bit t: Requirements.Compatible against template t fails (host verdict)
  const uint8_t* tcls;  // [T][TCLS_MAX] the template's taint classes in its NodePool's taint order, TCLS_END after
  uint32_t* cur;        // [nv][T][R] Fits threshold cursors
  uint32_t* out;        // [nv][T] packed words (explain_rules.hpp pack)
  uint32_t nv;
};

// <U> resources.Fits(Merge(daemon, pod), allocatable): the first threshold >=
// the demand, one lane per (variant, template, resource)
__global__ __launch_bounds__(BLOCK) void explain_cursor_kernel(DevProblem d, ExplainArgs a) {
  const uint32_t R = d.R, T = d.T;
  const uint64_t id = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (id >= (uint64_t)a.nv * T * R) return;
  const uint32_t r = (uint32_t)(id % R);
  const uint64_t pair = id / R;
  const uint32_t v = a.ev[pair / T], t = (uint32_t)(pair % T);
  const int64_t dem = d.tmpl[t].daemon[r] + d.pod_req[(size_t)d.var_pod[v] * R + r];
  const uint32_t o = d.thr_off[r];
  a.cur[id] = o + r + lower_bound_i64(d.thr_val + o, d.thr_off[r + 1] - o, dem);
}

// A wave holds PP = 64 / LP pairs: lane group s (LP lanes, LP = the row's word
// count rounded up to a power of two, at most 64) judges pair s, lane wl of
// the group the row words wl, wl + LP, ... (two at most: W <= 128).  Per word
//   S  the template's options (within the NodePool's limits as given)
//   R  the variant's instance-type requirement class mask
//   F  AND_r thr_set[r][cursor_r]
//   O  OR over the merged (zone, capacity type) grid of slot_set[g]
// and the booleans are "some word has a bit" of S&R, S&F, S&O, the three
// exactly-two terms and S&R&F&O, OR-reduced over the group by ballots.  S
// never has a bit at or beyond N, and every term starts from S, so the
// complements cannot count padding; the last word is masked all the same.
template <uint32_t LP>
__global__ __launch_bounds__(BLOCK) void explain_kernel(DevProblem d, ExplainArgs a) {
  constexpr uint32_t PP = 64 / LP;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t sub = lane / LP, wl = lane % LP;
  const uint32_t W = d.W, OW = d.OW, R = d.R, T = d.T;
  const uint32_t NP = a.nv * T;
  const uint32_t pair0 = __builtin_amdgcn_readfirstlane((blockIdx.x * (BLOCK / 64) + wv) * PP);
  if (pair0 >= NP) return;  // wave-uniform
  const uint32_t pair = pair0 + sub;
  const bool valid = pair < NP;
  const uint32_t i = valid ? pair / T : 0, t = valid ? pair % T : 0;
  const uint32_t v = a.ev[i];
  const VarRec& vr = d.vars[v];
  const TmplRec& tr = d.tmpl[t];
  const uint64_t unt = tr.taints & ~vr.tol;  // <U> Taints.ToleratesPod
  // <U> Requirements.Compatible: the free keys here (K1's check), every key on the host
  const bool incompat = !var_fk_ok(d, vr, d.t_fk + (size_t)t * d.F) || ((a.inc[i] >> t) & 1);
  const uint64_t G = grid_of(tr.zm & vr.zm, tr.cm & vr.cm, d.Z, d.C);
  const uint32_t itc = d.var_itclass[v];
  const uint64_t* itmask = itc != NONE ? d.itclass_mask + (size_t)itc * W : nullptr;
  const uint64_t* topts = (tr.has_limits ? d.t_limopts : d.t_opts) + (size_t)t * W;
  uint32_t cur[RMAX];
#pragma unroll
  for (uint32_t r = 0; r < RMAX; r++) cur[r] = valid && r < R ? a.cur[(size_t)pair * R + r] : 0u;

  uint32_t m = 0;               // this lane's booleans; bit 7: S has a bit
  uint64_t allw[2] = {0, 0};    // this lane's words of S & R & F & O (minValues)
  for (uint32_t w0 = 0, k = 0; w0 < W; w0 += LP, k++) {
    const uint32_t w = w0 + wl;
    if (!valid || w >= W) continue;
    const uint64_t vm = (w == W - 1 && (d.N & 63)) ? (1ull << (d.N & 63)) - 1 : ~0ull;
    const uint64_t S = topts[w] & vm;
    uint64_t F = ~0ull, O = 0;
#pragma unroll
    for (uint32_t r = 0; r < RMAX; r++)
      if (r < R) F &= d.thr_set[(size_t)cur[r] * OW + w];
    for (uint64_t g = G; g; g &= g - 1) O |= d.slot_set[(size_t)(__ffsll((long long)g) - 1) * W + w];
    const uint64_t Rm = itmask ? itmask[w] : ~0ull;
    const uint64_t sr = S & Rm, sf = S & F, so = S & O, all = sr & F & O;
    m |= (sr ? gsx::MET_REQUIREMENTS : 0u) | (sf ? gsx::MET_FITS : 0u) | (so ? gsx::MET_OFFERING : 0u) |
         ((sr & F & ~O) ? gsx::MET_REQ_FITS_ONLY : 0u) | ((sr & O & ~F) ? gsx::MET_REQ_OFFERING_ONLY : 0u) |
         ((sf & O & ~Rm) ? gsx::MET_FITS_OFFERING_ONLY : 0u) | (all ? gsx::MET_ALL : 0u) | (S ? 0x80u : 0u);
    if (k < 2) allw[k] = all;
  }
  // OR over the group: one ballot per boolean (every lane of the wave takes part)
  const uint64_t gmask = (LP == 64 ? ~0ull : ((1ull << LP) - 1)) << (sub * LP);
  uint32_t met = 0;
#pragma unroll
  for (uint32_t b = 0; b < 8; b++)
    if (__ballot((m >> b) & 1) & gmask) met |= 1u << b;

  // <U> minValues (Strict) on the options that met all three: mv_rows_kernel's
  // rule (distinct values per minimum key; a key whose value differs for every
  // type counts types).  Uniform trip count: the reductions run in every lane.
  bool mv_fail = false;
  if (d.any_mv) {
    for (uint32_t k = 0; k < (uint32_t)KMAX_IT; k++) {
      const bool on = valid && ((tr.mv_mask >> k) & 1);
      uint32_t n = 0;
      uint64_t sv[4] = {0, 0, 0, 0};
      if (on) {
        if ((d.it_key_unique >> k) & 1) {
          n = (uint32_t)__popcll(allw[0]) + (uint32_t)__popcll(allw[1]);
        } else {
          const uint16_t* dv = d.it_dvid + (size_t)k * d.N;
#pragma unroll
          for (uint32_t q = 0; q < 2; q++) {
            const uint32_t w = wl + q * LP;
            for (uint64_t x = allw[q]; x; x &= x - 1) {
              const uint32_t y = dv[w * 64 + (uint32_t)__builtin_ctzll(x)];
#pragma unroll
              for (uint32_t z = 0; z < 4; z++) sv[z] |= (y >> 6) == z ? 1ull << (y & 63) : 0ull;
            }
          }
        }
      }
#pragma unroll
      for (uint32_t o = LP / 2; o >= 1; o >>= 1) {
        n += (uint32_t)__shfl_xor((int)n, (int)o);
#pragma unroll
        for (uint32_t z = 0; z < 4; z++) sv[z] |= shfl_xor_u64(sv[z], (int)o);
      }
      if (on && !((d.it_key_unique >> k) & 1))
        n = (uint32_t)(__popcll(sv[0]) + __popcll(sv[1]) + __popcll(sv[2]) + __popcll(sv[3]));
      if (on && n < tr.mv[k]) mv_fail = true;
    }
  }

  if (!valid || wl != 0) return;
  uint32_t pos = 0;
  if (unt) {
    const uint8_t* tc = a.tcls + (size_t)t * TCLS_MAX;
    while (pos + 1 < TCLS_MAX && tc[pos] != TCLS_END && !((unt >> (tc[pos] & 63)) & 1)) pos++;
  }
  const uint32_t pre = (met & 0x80u ? 0u : gsx::PRE_LIMITS) | (unt ? gsx::PRE_TAINTS : 0u) |
                       (incompat ? gsx::PRE_INCOMPATIBLE : 0u) | (mv_fail ? gsx::PRE_MIN_VALUES : 0u);
  a.out[pair] = gsx::pack(met & gsx::MET_MASK, pre, pos);
}

template <uint32_t LP>
static void launch_lp(const DevProblem& d, const ExplainArgs& a, hipStream_t s) {
  const uint64_t pairs = (uint64_t)a.nv * d.T;
  const uint64_t per_block = (BLOCK / 64) * (64 / LP);
  hipLaunchKernelGGL(explain_kernel<LP>, dim3((uint32_t)((pairs + per_block - 1) / per_block)), dim3(BLOCK), 0, s, d, a);
}

static hipError_t launch(const DevProblem& d, const ExplainArgs& a, hipStream_t s) {
  const uint64_t nc = (uint64_t)a.nv * d.T * d.R;
  if (nc) hipLaunchKernelGGL(explain_cursor_kernel, dim3((uint32_t)((nc + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, d, a);
  const uint32_t W = d.W;
  if (W <= 1) launch_lp<1>(d, a, s);
  else if (W <= 2) launch_lp<2>(d, a, s);
  else if (W <= 4) launch_lp<4>(d, a, s);
  else if (W <= 8) launch_lp<8>(d, a, s);
  else if (W <= 16) launch_lp<16>(d, a, s);
  else if (W <= 32) launch_lp<32>(d, a, s);
  else launch_lp<64>(d, a, s);
  return hipGetLastError();
}

// the call's device buffers and pinned staging (they only grow) and the
// result storage the caller's gs_explain_result points into
struct State {
  gsc::DevBuf dev;
  gsc::PinnedBuf h_in, h_out;
  std::vector<uint32_t> pods;
  std::vector<uint8_t> cause, met;
  std::vector<int32_t> taint;
};

}  // namespace gse

using namespace gsc;
using namespace gse;

void gsc::explain_destroy(gs_ctx* c) {
  delete c->explain;  // its buffers with it
  c->explain = nullptr;
}

extern "C" uint32_t gs_explain_result_size(void) { return (uint32_t)sizeof(gs_explain_result); }

extern "C" gs_status gs_explain(gs_ctx* c, const uint32_t* pods, uint32_t n, uint32_t flags, gs_explain_result* out) {
  if (!c || !out) return GS_E_INVALID;
  if (!c->prepared) return fail(c, GS_E_INVALID, "gs_explain before gs_prepare");
  if (flags & ~GS_EXPLAIN_AS_GIVEN) return fail(c, GS_E_INVALID, "unknown gs_explain flag");
  if (!pods && n) return fail(c, GS_E_INVALID, "gs_explain: null pods with a non-zero count");
  const auto t0 = Clock::now();
  const auto& e = c->enc;
  const uint32_t P = e.P, T = e.T, NP = c->n_nodepools;
  // the list first, into memory of this call: it may point into the context's
  // last gs_result or into the previous explain result
  std::vector<uint32_t> list;
  if (!pods) {
    list.resize(P);
    for (uint32_t p = 0; p < P; p++) list[p] = p;
  } else {
    list.assign(pods, pods + n);
    for (uint32_t j = 0; j < n; j++)
      if (list[j] >= P)
        return fail(c, GS_E_INVALID, "gs_explain: pod index " + std::to_string(list[j]) + " out of range (" +
                                         std::to_string(P) + " pods)");
  }
  const uint32_t np_ = (uint32_t)list.size();
  // the distinct variants among them, in first-use order
  const bool as_given = flags & GS_EXPLAIN_AS_GIVEN;
  std::vector<uint32_t> ev, row_of(np_);
  {
    std::unordered_map<uint32_t, uint32_t> slot;
    slot.reserve(np_);
    for (uint32_t j = 0; j < np_; j++) {
      const uint32_t p = list[j];
      const uint32_t v = as_given ? e.var_begin[p] : e.var_begin[p] + e.var_count[p] - 1;
      auto f = slot.emplace(v, (uint32_t)ev.size());
      if (f.second) ev.push_back(v);
      row_of[j] = f.first->second;
    }
  }
  const uint32_t nv = (uint32_t)ev.size();
  std::vector<uint8_t> cause((size_t)np_ * NP, (uint8_t)gsx::WHY_NO_OPTIONS), met((size_t)np_ * NP, 0);
  std::vector<int32_t> taint((size_t)np_ * NP, -1);
  float kernel_ms = 0;
  uint64_t d2h = 0;
  if (nv && T) {
    // <U> Requirements.Compatible(pod, AllowUndefinedWellKnownLabels) against
    // each template, once per (spec variant, template): the full-vocabulary
    // algebra of reqs.cpp tells "template zone In [a], pod zone In [b]"
    // (incompatible) from "pod names a zone no offering has" (compatible; no
    // option has the offering), which the catalog-zone masks fold together
    std::vector<int8_t> memo(e.variants.size() * (size_t)T, -1);
    std::vector<uint64_t> inc(nv, 0);
    for (uint32_t i = 0; i < nv; i++) {
      const uint32_t sv = e.var_sv[ev[i]];
      for (uint32_t t = 0; t < T; t++) {
        int8_t& x = memo[(size_t)sv * T + t];
        if (x < 0) x = gsh::reqs_compatible(e, e.tmpl_reqs[t], e.variants[sv].reqs, true) ? 0 : 1;
        if (x) inc[i] |= 1ull << t;
      }
    }
    // per template: its taint classes in the NodePool's taint order (the first
    // taint of each class), and the taint each position stands for
    std::vector<uint8_t> tcls((size_t)T * TCLS_MAX, TCLS_END);
    std::vector<int32_t> pos_taint((size_t)T * TCLS_MAX, -1);
    for (uint32_t t = 0; t < T; t++) {
      uint64_t seen = 0;
      uint32_t k = 0;
      for (auto& tc : e.tmpl_taint_order[t]) {
        if ((seen >> tc.second) & 1) continue;
        seen |= 1ull << tc.second;
        tcls[(size_t)t * TCLS_MAX + k] = (uint8_t)tc.second;
        pos_taint[(size_t)t * TCLS_MAX + k] = (int32_t)tc.first;
        k++;
      }
    }
    const size_t pairs = (size_t)nv * T;
    const size_t ev_b = (size_t)nv * 4, inc_b = (size_t)nv * 8, tc_b = tcls.size();
    const size_t inc_off = up256(ev_b), tc_off = inc_off + up256(inc_b), in_bytes = tc_off + tc_b;
    const size_t cur_off = up256(in_bytes), out_off = cur_off + up256(pairs * std::max<uint32_t>(e.R, 1) * 4);
    const size_t out_bytes = pairs * 4, total = out_off + up256(out_bytes);
    try {
      HIPCHK(hipSetDevice(c->device));
      if (!c->explain) c->explain = new State;
      State& s = *c->explain;
      s.dev.reserve(total);
      s.h_in.reserve(in_bytes);
      s.h_out.reserve(out_bytes);
      char* hi = (char*)s.h_in.data();
      std::memcpy(hi, ev.data(), ev_b);
      std::memcpy(hi + inc_off, inc.data(), inc_b);
      std::memcpy(hi + tc_off, tcls.data(), tc_b);
      char* base = (char*)s.dev.data();
      HIPCHK(hipMemcpyAsync(base, hi, in_bytes, hipMemcpyHostToDevice, c->stream));
      ExplainArgs a{};
      a.ev = (const uint32_t*)base;
      a.inc = (const uint64_t*)(base + inc_off);
      a.tcls = (const uint8_t*)(base + tc_off);
      a.cur = (uint32_t*)(base + cur_off);
      a.out = (uint32_t*)(base + out_off);
      a.nv = nv;
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      HIPCHK(launch(c->dp, a, c->stream));
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      HIPCHK(hipMemcpyAsync(s.h_out.data(), base + out_off, out_bytes, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipEventElapsedTime(&kernel_ms, c->ev[6], c->ev[7]));
      d2h = out_bytes;
    } catch (const HipError& ex) {
      return fail(c, GS_E_HIP, ex.msg);
    }
    // the evaluated pairs -> the requested pods' rows
    const uint32_t* words = (const uint32_t*)c->explain->h_out.data();
    for (size_t q = 0; q < pairs; q++)
      if (gsx::packed_cause(words[q]) >= gsx::WHY_COUNT || gsx::packed_cause(words[q]) == gsx::WHY_NO_OPTIONS)
        return fail(c, GS_E_HIP, "gs_explain: a cause code outside the table came back");
    for (uint32_t j = 0; j < np_; j++)
      for (uint32_t t = 0; t < T; t++) {
        const uint32_t w = words[(size_t)row_of[j] * T + t];
        const size_t dst = (size_t)j * NP + e.tmpl[t].np_index;
        cause[dst] = (uint8_t)gsx::packed_cause(w);
        met[dst] = (uint8_t)gsx::packed_met(w);
        const uint32_t pos = gsx::packed_taint_pos(w);
        if (cause[dst] == gsx::WHY_TAINTS && pos < TCLS_MAX) taint[dst] = pos_taint[(size_t)t * TCLS_MAX + pos];
      }
  }
  if (!c->explain) c->explain = new State;
  State& s = *c->explain;
  s.pods.swap(list);
  s.cause.swap(cause);
  s.met.swap(met);
  s.taint.swap(taint);
  std::memset(out, 0, sizeof(*out));
  out->n_pods = np_;
  out->n_nodepools = NP;
  out->pods = s.pods.data();
  out->cause = s.cause.data();
  out->met = s.met.data();
  out->taint = s.taint.data();
  out->n_variants = (np_ && T) ? nv : 0;
  out->t_kernel_ms = kernel_ms;
  out->d2h_bytes = d2h;
  out->t_total_ms = ms_since(t0);
  return GS_OK;
}
