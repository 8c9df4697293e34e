// rank_batch.hip — autoplacement ranking against a catalog kept on the device
// (gs_rank_prepare / gs_rank_run / gs_rank_last_run, C-ABI in
// include/gpusched.h): IBMInstanceTypeProvider.FilterInstanceTypes +
// rankInstanceTypes (pkg/providers/common/instancetype/instancetype.go:259-379)
// for many IBMNodeClasses per launch, as the autoplacement controller asks it
// once per NodeClass (pkg/controllers/nodeclass/autoplacement/controller.go:104-163).
//
// calculateInstanceTypeScore (:90-110) reads only the type, never the query,
// so everything that depends on the catalog alone is done once, in prepare:
//   rank_prepare_kernel (grid-wide): per type the float64 score and a u16
//   key = how many scores OF THE CATALOG are strictly below it.
// key_i < key_j exactly when score_i < score_j, for every pair of types and so
// for every kept subset; Go's sort.Slice (pdqsort_func) depends only on Less
// outcomes, so sorting a query's kept (key, List index) pairs, compacted in
// List order, gives the reference's permutation, ties included.  This is
// rank_key_kernel's argument (rank.hip) with the count taken over the catalog
// instead of over the kept set.
//
// A run is one launch, rank_batch_kernel, one 64-thread workgroup (one wave)
// per query:
//   1. the four filters (rank_rules.hpp) over the resident columns; kept
//      key | index << 16 pairs go to LDS in List order with a ballot prefix;
//   2. the wave sorts them with the single-wave sort.Slice restatement
//      (ffd_wave.hpp wave_pdqsort, called as rank_sort_kernel calls it);
//   3. the first min(kept, stride) List indices go to the query's row, with
//      the resident scores beside them under GS_RANK_SCORES, and the count.
// One wave per workgroup: the sort is barrier-free by construction (every
// hand-off goes through the wave's in-order LDS queue), so the whole kernel
// has no workgroup barrier, and nq workgroups spread over the CUs; with 256
// threads three waves would only wait at a barrier while the first sorts.
// LDS per workgroup: 6 B per catalog type + 4 B (24 KB at 4,096 types; the
// sorter keeps its frames in VGPR lanes, so the Frame[64] array its signature
// takes is dropped by the compiler), under the 64 KB default: no attribute
// call, and at CM's 198 types 1.2 KB, so LDS never limits the waves per CU.
//
// HBM, resident: cpu i64 | mem i64 | price f64 | arch u32 (uploaded, 28 B per
// type) | score f64 | key u16 (computed).  A run uploads 32 B per query and
// reads back [score f64 [nq][stride]] | order u32 [nq][stride] | kept u32 [nq].
//
// The host side lives in this unit too (it needs the HIP runtime).
#include "ffd_wave.hpp"

#include "ctx.hpp"
#include "rank_rules.hpp"

static_assert(gsr::kArchAny == GS_ARCH_ANY, "rank_rules.hpp arch wildcard");
static_assert(sizeof(gs_rank_query) == 32 && offsetof(gs_rank_query, max_price) == 16 &&
                  offsetof(gs_rank_query, want_arch) == 24,
              "gs_rank_query is read by the kernel as it is");
static_assert(GS_RANK_MAX <= 65536u, "a List index rides in 16 bits beside its key");

namespace gsrb {

using gsc::HipError;

constexpr uint32_t RP_NT = 256;
constexpr uint32_t RP_NWAVE = RP_NT / 64;

// the resident catalog (device pointers into one allocation)
struct DevCatalog {
  const int64_t* cpu_milli;
  const int64_t* memory_bytes;
  const double* price;
  const uint32_t* arch;
  double* score;
  uint16_t* key;
  uint32_t n;
};

// Workgroup b owns types [64b, 64b + 64) (lane = type).  Every workgroup
// scores the whole catalog into LDS (n <= 4096: cheaper than a second launch
// or a grid-wide wait), its 4 waves split the j range of the strictly-below
// count (a broadcast LDS read per j) and add their partial counts in LDS.
__global__ __launch_bounds__(RP_NT) void rank_prepare_kernel(DevCatalog d) {
  extern __shared__ double rp_all[];  // [n] scores
  __shared__ uint32_t part[RP_NWAVE][64];
  const uint32_t n = d.n;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t k = blockIdx.x * 64u + lane;
  for (uint32_t j = threadIdx.x; j < n; j += RP_NT)
    rp_all[j] = gsr::score(d.cpu_milli[j], d.memory_bytes[j], d.price[j]);
  __syncthreads();
  const double x = k < n ? rp_all[k] : 0.0;
  const uint32_t per = (n + RP_NWAVE - 1) / RP_NWAVE;
  const uint32_t j0 = wave * per < n ? wave * per : n, j1 = j0 + per < n ? j0 + per : n;
  uint32_t below = 0;
#pragma unroll 8
  for (uint32_t j = j0; j < j1; j++) below += rp_all[j] < x;
  part[wave][lane] = below;
  __syncthreads();
  if (wave == 0 && k < n) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < RP_NWAVE; w++) t += part[w][lane];
    d.score[k] = x;
    d.key[k] = (uint16_t)t;  // < n <= 4096
  }
}

struct DevRun {
  const gs_rank_query* q;
  uint32_t* out_order;  // [nq][stride]
  double* out_score;    // [nq][stride], or nullptr
  uint32_t* out_kept;   // [nq]
  uint32_t stride;
};

__global__ __launch_bounds__(64) void rank_batch_kernel(DevCatalog d, DevRun r) {
  extern __shared__ uint32_t rb_lds[];  // so[n] (key | List index << 16) | scr u16[n + 2]
  __shared__ Frame rb_stk[64];
  const uint32_t lane = threadIdx.x;
  const uint32_t n = d.n;
  const gs_rank_query Q = r.q[blockIdx.x];
  lds_u32* so = (lds_u32*)rb_lds;
  lds_u16* scr = (lds_u16*)(rb_lds + n);
  uint32_t kept = 0;
  for (uint32_t c = 0; c < n; c += 64) {
    const uint32_t i = c + lane;
    const bool keep = i < n && gsr::keep(d.cpu_milli[i], d.memory_bytes[i], d.price[i], d.arch[i], Q.want_arch,
                                         Q.min_cpu, Q.min_memory_gb, Q.max_price);
    const uint64_t b = __ballot(keep);
    if (keep) so[kept + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)d.key[i] | (i << 16);
    kept += (uint32_t)__popcll(b);  // <= n: every pair lands inside so[0, n)
  }
  kept = __builtin_amdgcn_readfirstlane(kept);
  wsync();
  wave_pdqsort<GS_WAVE_SEQ, lds_u32, lds_u16, false, true>(so, scr, (lds_frame*)rb_stk, lane, (kept + 1) / 2, (int)kept,
                                                          -1);
  wsync();
  const uint32_t m = kept < r.stride ? kept : r.stride;
  const size_t row = (size_t)blockIdx.x * r.stride;
  for (uint32_t k = lane; k < m; k += 64) {
    const uint32_t i = so[k] >> 16;  // < n
    r.out_order[row + k] = i;
    if (r.out_score) r.out_score[row + k] = d.score[i];
  }
  if (lane == 0) r.out_kept[blockIdx.x] = kept;
}

// everything the resident ranking keeps in a context (gs_ctx::rank, made on first use)
struct State {
  bool ready = false;
  gsc::DevBuf cat_dev;
  DevCatalog cat{};
  // a run's queries and outputs: grow-once device arena, pinned host sides
  gsc::DevBuf run_dev;
  gsc::PinnedBuf h_in, h_out;
  gs_rank_stats stats{};
};

static State& state(gs_ctx* c) {
  if (!c->rank) c->rank = new State;
  return *c->rank;
}

}  // namespace gsrb

using namespace gsc;
using namespace gsrb;

void gsc::rank_batch_destroy(gs_ctx* c) {
  delete c->rank;  // its buffers with it
  c->rank = nullptr;
}

extern "C" uint32_t gs_rank_query_size(void) { return (uint32_t)sizeof(gs_rank_query); }
extern "C" uint32_t gs_rank_result_size(void) { return (uint32_t)sizeof(gs_rank_result); }
extern "C" uint32_t gs_rank_stats_size(void) { return (uint32_t)sizeof(gs_rank_stats); }

extern "C" gs_status gs_rank_last_run(const gs_ctx* c, gs_rank_stats* out) {
  if (!c || !out) return GS_E_INVALID;
  *out = c->rank ? c->rank->stats : gs_rank_stats{};
  return GS_OK;
}

extern "C" gs_status gs_rank_prepare(gs_ctx* c, uint32_t n, const int64_t* cpu_milli, const int64_t* memory_bytes,
                                     const double* price, const uint32_t* arch) {
  if (!c) return GS_E_INVALID;
  // the checks of gs_rank_instance_types, on the host before the device is
  // touched: a failure leaves the resident catalog as it was
  if (n && (!cpu_milli || !memory_bytes || !price || !arch))
    return fail(c, GS_E_INVALID, "gs_rank_prepare: null column with a non-zero count");
  if (n > GS_RANK_MAX) return fail(c, GS_E_CAPACITY, "gs_rank_prepare: more than GS_RANK_MAX instance types");
  for (uint32_t i = 0; i < n; i++)
    if (cpu_milli[i] < 0 || memory_bytes[i] < 0 || price[i] != price[i])  // NaN price
      return fail(c, GS_E_INVALID, "gs_rank_prepare: negative quantity or NaN price at instance type " + std::to_string(i));
  const auto t0 = Clock::now();
  const size_t nn = n;
  // cpu | mem | price (8 B each) | arch (4 B): one transfer; then score | key
  const size_t in_bytes = nn * 28;
  const size_t score_off = up256(in_bytes), key_off = score_off + up256(nn * 8);
  const size_t bytes = key_off + up256(nn * 2) + 256;
  std::vector<char> h(in_bytes);
  if (n) {
    std::memcpy(h.data(), cpu_milli, nn * 8);
    std::memcpy(h.data() + nn * 8, memory_bytes, nn * 8);
    std::memcpy(h.data() + nn * 16, price, nn * 8);
    std::memcpy(h.data() + nn * 24, arch, nn * 4);
  }
  const double encode_ms = ms_since(t0);
  const auto t1 = Clock::now();
  DevBuf image;  // the new catalog: freed by scope on a failure
  DevCatalog d{};
  float kernel_ms = 0;
  try {
    HIPCHK(hipSetDevice(c->device));
    image.reserve_exact(bytes);
    char* dev = (char*)image.data();
    d.cpu_milli = (const int64_t*)dev;
    d.memory_bytes = (const int64_t*)(dev + nn * 8);
    d.price = (const double*)(dev + nn * 16);
    d.arch = (const uint32_t*)(dev + nn * 24);
    d.score = (double*)(dev + score_off);
    d.key = (uint16_t*)(dev + key_off);
    d.n = n;
    if (n) {
      HIPCHK(hipMemcpyAsync(dev, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      hipLaunchKernelGGL(rank_prepare_kernel, dim3((n + 63) / 64), dim3(RP_NT), nn * sizeof(double), c->stream, d);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));  // also: no run of the old catalog is in flight
    if (n) HIPCHK(hipEventElapsedTime(&kernel_ms, c->ev[6], c->ev[7]));
  } catch (const HipError& ex) {
    return fail(c, GS_E_HIP, ex.msg);
  }
  State& s = state(c);
  s.cat_dev = std::move(image);  // frees the old catalog
  s.cat = d;
  s.ready = true;
  s.stats = gs_rank_stats{};
  s.stats.encode_ms = encode_ms;
  s.stats.upload_ms = ms_since(t1);
  s.stats.kernel_ms = kernel_ms;
  s.stats.h2d_bytes = in_bytes;
  s.stats.n_launches = n ? 1 : 0;
  s.stats.n_instance_types = n;
  return GS_OK;
}

extern "C" gs_status gs_rank_run(gs_ctx* c, const gs_rank_query* q, uint32_t nq, uint32_t max_out, uint32_t flags,
                                 gs_rank_result* out) {
  if (!c || !out) return GS_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (!c->rank || !c->rank->ready) return fail(c, GS_E_INVALID, "gs_rank_run before gs_rank_prepare");
  if (nq && !q) return fail(c, GS_E_INVALID, "gs_rank_run: null queries with a non-zero count");
  if (flags & ~GS_RANK_SCORES) return fail(c, GS_E_INVALID, "unknown gs_rank_run flag");
  if (nq > GS_RANK_BATCH_MAX) return fail(c, GS_E_CAPACITY, "more than GS_RANK_BATCH_MAX queries in one gs_rank_run call");
  State& s = *c->rank;
  const auto t0 = Clock::now();
  const uint32_t n = s.cat.n;
  const uint32_t stride = max_out ? std::min(max_out, n) : n;
  const bool scores = flags & GS_RANK_SCORES;
  gs_rank_stats st{};
  st.n_queries = nq;
  st.n_instance_types = n;
  const uint32_t* h_kept = nullptr;
  const uint32_t* h_order = nullptr;
  const double* h_score = nullptr;
  if (nq) {
    try {
      HIPCHK(hipSetDevice(c->device));
      const size_t cells = (size_t)nq * stride;
      const size_t in_bytes = (size_t)nq * sizeof(gs_rank_query);
      const size_t score_bytes = scores ? cells * 8 : 0;
      const size_t out_bytes = score_bytes + cells * 4 + (size_t)nq * 4;  // scores | order | kept
      const size_t out_off = up256(in_bytes);
      s.run_dev.reserve(out_off + out_bytes);
      s.h_in.reserve(in_bytes);
      s.h_out.reserve(out_bytes);
      std::memcpy(s.h_in.data(), q, in_bytes);
      st.encode_ms = ms_since(t0);
      const auto t1 = Clock::now();
      char* base = (char*)s.run_dev.data();
      HIPCHK(hipMemcpyAsync(base, s.h_in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
      st.h2d_bytes = in_bytes;
      DevRun r{};
      r.q = (const gs_rank_query*)base;
      r.out_score = scores ? (double*)(base + out_off) : nullptr;
      r.out_order = (uint32_t*)(base + out_off + score_bytes);
      r.out_kept = r.out_order + cells;
      r.stride = stride;
      const size_t lds = (size_t)n * sizeof(uint32_t) + ((size_t)n + 2) * sizeof(uint16_t);
      HIPCHK(hipEventRecord(c->ev[6], c->stream));
      hipLaunchKernelGGL(rank_batch_kernel, dim3(nq), dim3(64), lds, c->stream, s.cat, r);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[7], c->stream));
      st.n_launches = 1;
      st.upload_ms = ms_since(t1);
      const auto t2 = Clock::now();
      HIPCHK(hipMemcpyAsync(s.h_out.data(), base + out_off, out_bytes, hipMemcpyDeviceToHost, c->stream));
      st.d2h_bytes = out_bytes;
      HIPCHK(hipStreamSynchronize(c->stream));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
      st.kernel_ms = ms;
      const char* ho = (const char*)s.h_out.data();
      h_score = scores ? (const double*)ho : nullptr;
      h_order = (const uint32_t*)(ho + score_bytes);
      h_kept = h_order + cells;
      for (uint32_t i = 0; i < nq; i++)
        if (h_kept[i] > n) return fail(c, GS_E_HIP, "gs_rank_run: a kept count above the catalog's size came back");
      st.fetch_ms = ms_since(t2);
    } catch (const HipError& ex) {
      return fail(c, GS_E_HIP, ex.msg);
    }
  } else {
    st.encode_ms = ms_since(t0);
  }
  s.stats = st;
  out->n_queries = nq;
  out->stride = stride;
  out->n_kept = h_kept;
  out->order = h_order;
  out->score = h_score;
  return GS_OK;
}
