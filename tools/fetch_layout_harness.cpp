// fetch_layout_harness.cpp — gs_batch_fetch_all's layout arithmetic and record
// validation (csrc/batch_fetch_layout.hpp) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined tools/fetch_layout_harness.cpp
// It includes that header and nothing else of the library.
//
// usage: fetch_layout_harness <case>
// A case builds a gathered buffer as the device writes it (heads and payload in
// heap blocks of exactly the transferred size, so a read past either is a
// sanitizer report), optionally corrupts it, runs gsbf::validate and then reads
// every byte of every region of every slot that passed, as the decoder would.
// Output: one line "n=<slots> good=<passed> ok=<one digit per slot>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../karpenter-provider-ibm-cloud_amd/csrc/batch_fetch_layout.hpp"

using namespace gsbf;

namespace {

struct Slot {
  uint32_t n_log, n_claims, qlen;  // what the Solve left
  uint32_t P, claim_cap;           // the slot's bounds
  uint32_t status = 0;
};

struct Buffer {
  std::vector<FetchHead> heads;
  std::vector<FetchBounds> bounds;
  uint64_t total = 0;  // FetchTop::total
  uint64_t have = 0;   // payload bytes transferred
};

// the sizing pass: heads with an exclusive prefix sum in slot order
Buffer build(const std::vector<Slot>& slots) {
  Buffer b;
  uint64_t run = 0;
  for (const Slot& s : slots) {
    FetchHead h{};
    h.status = s.status;
    h.n_log = s.n_log;
    h.n_claims = s.n_claims;
    h.qlen = s.qlen;
    if (s.n_log > s.P || s.n_claims > s.claim_cap || s.qlen > s.P)
      h.flags = FH_CORRUPT;
    else if (s.status == 0)
      h.bytes = payload_bytes(s.n_log, s.n_claims, s.qlen);
    h.off = run;
    run += h.bytes;
    b.heads.push_back(h);
    b.bounds.push_back(FetchBounds{s.P, s.claim_cap});
  }
  b.total = b.have = run;
  return b;
}

int run(const Buffer& b) {
  const uint32_t n = (uint32_t)b.heads.size();
  // exact-size heap copies: what the host holds after the transfer
  FetchHead* heads = (FetchHead*)std::malloc(n ? n * sizeof(FetchHead) : 1);
  if (n) std::memcpy(heads, b.heads.data(), n * sizeof(FetchHead));
  unsigned char* payload = (unsigned char*)std::malloc(b.have ? b.have : 1);
  for (uint64_t i = 0; i < b.have; i++) payload[i] = (unsigned char)(i * 131u);
  std::vector<uint8_t> ok(n ? n : 1, 0);
  const uint32_t good = validate(heads, b.bounds.data(), n, b.total, b.have, ok.data());
  uint64_t sum = 0;
  for (uint32_t p = 0; p < n; p++) {
    if (!ok[p]) continue;
    const FetchHead& h = heads[p];
    if (h.status != 0) continue;  // a failed Solve has no records to read
    const FetchRegions r = regions(h.n_log, h.n_claims, h.qlen);
    const unsigned char* pay = payload + h.off;
    for (uint64_t i = r.log; i < r.rec; i++) sum += pay[i];
    for (uint64_t i = r.rec; i < r.its; i++) sum += pay[i];
    for (uint64_t i = r.its; i < r.nits; i++) sum += pay[i];
    for (uint64_t i = r.nits; i < r.nits + (uint64_t)h.n_claims * 4; i++) sum += pay[i];
    for (uint64_t i = r.unplaced; i < r.unplaced + (uint64_t)h.qlen * 4; i++) sum += pay[i];
  }
  std::string bits;
  for (uint32_t p = 0; p < n; p++) bits += ok[p] ? '1' : '0';
  std::printf("n=%u good=%u ok=%s sum=%llu\n", n, good, bits.c_str(), (unsigned long long)sum);
  std::free(payload);
  std::free(heads);
  return 0;
}

const std::vector<Slot> kThree = {{5, 2, 1, 8, 4}, {0, 0, 7, 7, 3}, {9, 3, 0, 9, 3}};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: fetch_layout_harness <case>\n");
    return 2;
  }
  const std::string c = argv[1];
  // ---- layout arithmetic
  if (c == "arithmetic") {
    static_assert(payload_base(0) == 64 && payload_base(1) == 192 && payload_base(3) == 448, "payload base");
    static_assert(payload_bytes(0, 0, 0) == 0, "empty slot");
    static_assert(payload_bytes(1, 0, 0) == 16 && payload_bytes(0, 0, 1) == 16 && payload_bytes(0, 0, 5) == 32, "units");
    static_assert(payload_bytes(0, 1, 0) == 192 + 240 + 16, "one NodeClaim");
    static_assert(payload_bytes(3, 5, 2) == 48 + 5 * 432 + 32 + 16, "mixed");
    const FetchRegions r = regions(3, 5, 2);
    const bool aligned = !(r.log % 16) && !(r.rec % 16) && !(r.its % 16) && !(r.nits % 16) && !(r.unplaced % 16) && !(r.end % 16);
    // 4,096 slots of the largest Solve: no 64-bit overflow
    const uint64_t big = worst_bytes(FetchBounds{0xFFFFFFFFu, 65535u});
    std::printf("aligned=%d big_ok=%d\n", aligned ? 1 : 0, big < (1ull << 50) ? 1 : 0);
    return 0;
  }
  // ---- buffers the validation must accept
  if (c == "valid0") return run(build({}));
  if (c == "valid1") return run(build({{5, 2, 1, 8, 4}}));
  if (c == "valid3") return run(build(kThree));  // the last slot ends exactly at the buffer end
  if (c == "valid_empty") return run(build({{0, 0, 0, 0, 1}, {4, 1, 0, 4, 1}, {0, 0, 0, 3, 2}}));  // P = 0; nothing placed
  if (c == "valid_failed_solve") {
    std::vector<Slot> s = kThree;
    s[1].status = 1;  // ST_CLAIMS: a head, no payload
    return run(build(s));
  }
  if (c == "valid_hint_larger") {
    // the transfer carried more than the run left (a larger earlier total)
    Buffer b = build(kThree);
    b.have += 4096;
    return run(b);
  }
  // ---- corruptions: the slot named fails alone, nothing is read out of bounds
  Buffer b = build(kThree);
  if (c == "offset_past_end") {
    b.heads[2].off = b.have + 16;
  } else if (c == "offset_wraps") {
    b.heads[2].off = ~(uint64_t)15u;
  } else if (c == "size_over_bound_log") {
    b.heads[0].n_log = 9;  // P = 8
    b.heads[0].bytes = payload_bytes(9, 2, 1);
  } else if (c == "size_over_bound_claims") {
    b.heads[2].n_claims = 4;  // claim_cap = 3
    b.heads[2].bytes = payload_bytes(9, 4, 0);
  } else if (c == "size_over_bound_queue") {
    b.heads[1].qlen = 0x40000001u;  // P = 7
  } else if (c == "flagged") {
    b.heads[1].flags = FH_CORRUPT;
  } else if (c == "bytes_mismatch") {
    b.heads[0].bytes -= 16;
  } else if (c == "overlap") {
    b.heads[2].off = b.heads[0].off + 16;  // inside slot 0's region
  } else if (c == "unaligned") {
    b.heads[2].off += 4;
  } else if (c == "total_small") {
    b.total = b.heads[2].off + b.heads[2].bytes - 16;  // smaller than the sum: the last slot is cut
  } else if (c == "transfer_short") {
    b.have = b.heads[2].off + 32;  // the mirror holds less than the total says
  } else {
    std::fprintf(stderr, "unknown case %s\n", c.c_str());
    return 2;
  }
  return run(b);
}
