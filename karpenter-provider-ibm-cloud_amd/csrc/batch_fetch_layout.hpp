// batch_fetch_layout.hpp — the staging buffer of gs_batch_fetch_all: what the
// gather kernels (batch_fetch.hip) write, what the host (batch.cpp) transfers,
// checks and decodes.  Host-only arithmetic: no HIP include, no other header of
// the library, so a plain g++ build can test it (tools/fetch_layout_harness.cpp).
//
//   [0, 64)                    FetchTop: the payload's total size
//   [64, 64 + n x 128)         FetchHead per gathered slot, in device array order
//   [payload_base(n), + total) each slot's records behind one another in the same
//                              order (an exclusive prefix sum over the slots, so
//                              the layout is the same from run to run)
//
// A slot's payload, every region 16-byte aligned:
//   LogRec[n_log]  ClaimRec[n_claims]  its[n_claims][60]  nits[n_claims]  unplaced[qlen]
// unplaced[i] is queue[(qhead + i) % P]: the ring is unrolled on the device.
// A slot whose Solve failed (status != 0) has no payload; a slot whose sizes
// exceed its own bounds is flagged FH_CORRUPT and has none either.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gsbf {

constexpr uint32_t kTopBytes = 64;
constexpr uint32_t kLogRecBytes = 16;     // sizeof(gsd::LogRec)
constexpr uint32_t kClaimRecBytes = 192;  // sizeof(gsd::ClaimRec)
constexpr uint32_t kItsRow = 60;          // instance types of a NodeClaim's OrderByPrice + Truncate(60) row
constexpr uint32_t kItsRowBytes = kItsRow * 4;
constexpr uint32_t kMaxSlots = 4096;      // GS_BATCH_MAX

enum : uint32_t { FH_CORRUPT = 1u };

struct FetchTop {
  uint64_t total;  // payload bytes of all slots
  uint32_t n;      // slots gathered
  uint32_t pad[13];
};
static_assert(sizeof(FetchTop) == kTopBytes, "FetchTop layout");

// the Ctrl fields gs_fetch reads (no dbg), and where the slot's records are
struct FetchHead {
  uint32_t status, n_claims, n_log, qlen;
  uint32_t qhead, flags;
  uint64_t off;    // first payload byte, relative to the payload base
  uint64_t bytes;  // payload_bytes(n_log, n_claims, qlen), 0 without payload
  uint64_t pops, generic_sorts, fast_sorts, cand_evals, cand_full, node_prefix, claim_prefix;
  uint64_t t_sort, t_scan, t_tmpl;
  uint64_t pad;
};
static_assert(sizeof(FetchHead) == 128, "FetchHead layout");

// what a slot's sizes may not exceed: its pods and its NodeClaim slots
struct FetchBounds {
  uint32_t P, claim_cap;
};

constexpr uint64_t align16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
constexpr uint64_t payload_base(uint32_t n) { return align16(kTopBytes + (uint64_t)n * sizeof(FetchHead)); }

// byte offsets of a slot's regions inside its payload
struct FetchRegions {
  uint64_t log, rec, its, nits, unplaced, end;
};
constexpr FetchRegions regions(uint32_t n_log, uint32_t n_claims, uint32_t qlen) {
  FetchRegions r{};
  r.log = 0;
  r.rec = r.log + (uint64_t)n_log * kLogRecBytes;
  r.its = r.rec + (uint64_t)n_claims * kClaimRecBytes;
  r.nits = r.its + (uint64_t)n_claims * kItsRowBytes;
  r.unplaced = r.nits + align16((uint64_t)n_claims * 4u);
  r.end = r.unplaced + align16((uint64_t)qlen * 4u);
  return r;
}
constexpr uint64_t payload_bytes(uint32_t n_log, uint32_t n_claims, uint32_t qlen) {
  return regions(n_log, n_claims, qlen).end;
}
// the most a slot can contribute (the host refuses a larger total as corrupt)
constexpr uint64_t worst_bytes(const FetchBounds& b) { return payload_bytes(b.P, b.claim_cap, b.P); }

inline bool within(const FetchHead& h, const FetchBounds& b) {
  return h.n_log <= b.P && h.n_claims <= b.claim_cap && h.qlen <= b.P;
}

// Which gathered slots may be decoded.  `have` is the number of payload bytes
// the host holds (transferred), `total` the FetchTop's.  ok[p] = 1 when slot
// p's head is not flagged, its sizes are within its bounds, its byte count is
// what its sizes give, its region is 16-byte aligned, lies inside
// min(total, have) and starts at or after the end of every earlier slot's
// region that passed (slots lie in device array order).  A slot that fails
// leaves the others alone.  Returns how many slots passed.
inline uint32_t validate(const FetchHead* heads, const FetchBounds* bounds, uint32_t n, uint64_t total, uint64_t have,
                         uint8_t* ok) {
  const uint64_t limit = total < have ? total : have;
  uint64_t floor = 0;  // end of the furthest sound region so far
  uint32_t good = 0;
  for (uint32_t p = 0; p < n; p++) {
    const FetchHead& h = heads[p];
    ok[p] = 0;
    if (h.flags & FH_CORRUPT) continue;
    if (!within(h, bounds[p])) continue;
    const uint64_t want = h.status == 0 ? payload_bytes(h.n_log, h.n_claims, h.qlen) : 0;
    if (h.bytes != want) continue;
    if (h.off & 15u) continue;
    if (h.off > limit || h.bytes > limit - h.off) continue;
    if (h.bytes && h.off < floor) continue;
    if (h.off + h.bytes > floor) floor = h.off + h.bytes;
    ok[p] = 1;
    good++;
  }
  return good;
}

}  // namespace gsbf
