// explain_rules_harness.cpp — csrc/explain_rules.hpp on the CPU, alone.
//
// A stand-alone program (its own main) that includes nothing of the library
// but that header.  It walks all 128 combinations of the seven booleans times
// the 32 pre-check states and prints, per line,
//   <met> <pre> <cause> <met as reported> <packed word round trip ok>
// tests/test_explain_rules.py builds it with g++ -fsanitize=address,undefined,
// runs it directly and compares every line with the table written in Python.
#include <cstdio>

#include "../karpenter-provider-ibm-cloud_amd/csrc/explain_rules.hpp"

int main() {
  for (uint32_t met = 0; met <= gsx::MET_MASK; met++)
    for (uint32_t pre = 0; pre <= gsx::PRE_MASK; pre++) {
      const uint32_t cause = gsx::cause_of(met, pre);
      const uint32_t rep = gsx::met_reported(met, pre);
      bool ok = true;
      for (uint32_t pos = 0; pos < 64; pos++) {
        const uint32_t w = gsx::pack(met, pre, pos);
        ok = ok && gsx::packed_cause(w) == cause && gsx::packed_met(w) == rep &&
             gsx::packed_taint_pos(w) == (cause == gsx::WHY_TAINTS ? pos : 0xFFFFFFFFu);
      }
      std::printf("%u %u %u %u %d\n", met, pre, cause, rep, ok ? 1 : 0);
    }
  return 0;
}
