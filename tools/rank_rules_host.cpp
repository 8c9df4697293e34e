// rank_rules_host — the ranking's filter and score rules (csrc/rank_rules.hpp,
// the text both ranking kernels compile) evaluated on the CPU, for
// tests/test_rank_batch.py: built with g++ -fsanitize=address,undefined and
// run as a child process.
//
// stdin:  R Q
//         R rows    cpu_milli memory_bytes price_bits(hex) arch
//         Q queries want_arch min_cpu min_memory_gb max_price_bits(hex)
// stdout: per row one line: the score's 64-bit pattern (hex), then Q keep bits
// Doubles travel as bit patterns so that NaN and inf arrive as they were sent.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../karpenter-provider-ibm-cloud_amd/csrc/rank_rules.hpp"

namespace {

struct Row {
  int64_t cpu, mem;
  double price;
  uint32_t arch;
};
struct Query {
  uint32_t want_arch;
  int64_t min_cpu, min_mem;
  double max_price;
};

double from_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
uint64_t to_bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

}  // namespace

int main() {
  uint32_t R = 0, Q = 0;
  if (std::scanf("%" SCNu32 " %" SCNu32, &R, &Q) != 2 || R > 65536 || Q > 65536) return 2;
  std::vector<Row> rows(R);
  std::vector<Query> qs(Q);
  for (Row& r : rows) {
    uint64_t pb = 0;
    if (std::scanf("%" SCNd64 " %" SCNd64 " %" SCNx64 " %" SCNu32, &r.cpu, &r.mem, &pb, &r.arch) != 4) return 2;
    r.price = from_bits(pb);
  }
  for (Query& q : qs) {
    uint64_t pb = 0;
    if (std::scanf("%" SCNu32 " %" SCNd64 " %" SCNd64 " %" SCNx64, &q.want_arch, &q.min_cpu, &q.min_mem, &pb) != 4)
      return 2;
    q.max_price = from_bits(pb);
  }
  for (const Row& r : rows) {
    std::printf("%016" PRIx64, to_bits(gsr::score(r.cpu, r.mem, r.price)));
    for (const Query& q : qs)
      std::printf(" %d", gsr::keep(r.cpu, r.mem, r.price, r.arch, q.want_arch, q.min_cpu, q.min_mem, q.max_price) ? 1 : 0);
    std::printf("\n");
  }
  return 0;
}
