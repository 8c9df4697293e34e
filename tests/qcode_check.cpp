// qcode_check.cpp — csrc/qcode.hpp against the definitions it replaced.
// A stand-alone program (tests/test_qcode.py builds it with
// -fsanitize=undefined,address and runs it): every code through qcode_value,
// the listed values through qcode_floor and qcode_ceil, equality with the
// early-return definitions below, the bracketing
// qcode_value(qcode_floor(v)) <= v <= qcode_value(qcode_ceil(v)) for v > 0,
// and every code within 16 bits.  Exit status 0 and "ok" on success.
#include <stdint.h>
#include <stdio.h>

#include "qcode.hpp"

namespace ref {
// the definitions of ffd_common.hpp before the header (with the compiler's
// count-leading-zeros builtin for the device's __clzll)
uint32_t qcode_floor(int64_t v) {
  if (v <= 0) return 0;
  const uint64_t x = (uint64_t)v;
  const uint32_t b = 64u - (uint32_t)__builtin_clzll((long long)x);
  if (b <= 10) return (uint32_t)x;
  const uint32_t s = b - 10;
  return 1024u + (s - 1) * 512u + (uint32_t)((x >> s) - 512u);
}
uint32_t qcode_ceil(int64_t v) {
  if (v <= 0) return 0;
  const uint64_t x = (uint64_t)v;
  const uint32_t b = 64u - (uint32_t)__builtin_clzll((long long)x);
  if (b <= 10) return (uint32_t)x;
  const uint32_t s = b - 10;
  const uint32_t c = 1024u + (s - 1) * 512u + (uint32_t)((x >> s) - 512u);
  return c + ((x & ((1ull << s) - 1)) ? 1u : 0u);
}
// (defined for codes below 33,280; from there on the shift count is 64 or
// more, so main() does not call it there)
int64_t qcode_value(uint32_t c) {
  if (c < 1024u) return (int64_t)c;
  const uint32_t s = (c - 1024u) / 512u + 1u, m = (c - 1024u) % 512u + 512u;
  return (int64_t)((uint64_t)m << s);
}
}  // namespace ref

static uint64_t n_checked = 0, n_bad = 0;

static void bad(const char* what, int64_t v, uint64_t got, uint64_t want) {
  if (n_bad++ < 20) fprintf(stderr, "%s(%lld): %llu, reference %llu\n", what, (long long)v, (unsigned long long)got, (unsigned long long)want);
}

static void check_v(int64_t v) {
  const uint32_t f = qcode_floor(v), c = qcode_ceil(v);
  n_checked++;
  if (f != ref::qcode_floor(v)) bad("qcode_floor", v, f, ref::qcode_floor(v));
  if (c != ref::qcode_ceil(v)) bad("qcode_ceil", v, c, ref::qcode_ceil(v));
  if (f > 0xFFFFu) bad("qcode_floor over 16 bits", v, f, 0xFFFFu);
  if (c > 0xFFFFu) bad("qcode_ceil over 16 bits", v, c, 0xFFFFu);
  if (c < f || c > f + 1) bad("qcode_ceil not floor or floor + 1", v, c, f);
  if (v > 0) {
    // as the non-negative quantities they are: above 1023 * 2^53 the ceiling
    // code is the next binade's first, which stands for 2^63 (qcode_value
    // returns its bit pattern; no claim or node holds such a quantity)
    if ((uint64_t)qcode_value(f) > (uint64_t)v) bad("qcode_value(qcode_floor) above", v, (uint64_t)qcode_value(f), (uint64_t)v);
    if ((uint64_t)qcode_value(c) < (uint64_t)v) bad("qcode_value(qcode_ceil) below", v, (uint64_t)qcode_value(c), (uint64_t)v);
  }
}

int main() {
  // every code: equality with the replaced definition where that one is
  // defined (binade shift <= 63, codes below 33,280: every code a quantity
  // can have, qcode_ceil(INT64_MAX) is 28,160); above, the header's own rule,
  // mantissa << (shift modulo 64), worked out here without a variable shift
  // count that could leave 0..63
  for (uint32_t c = 0; c < 65536u; c++) {
    n_checked++;
    if (c < 33280u) {
      if (qcode_value(c) != ref::qcode_value(c)) bad("qcode_value", c, (uint64_t)qcode_value(c), (uint64_t)ref::qcode_value(c));
    } else {
      const uint32_t sh = ((c >> 9) - 1u) % 64u;
      uint64_t want = (c & 511u) + 512u;
      for (uint32_t k = 0; k < sh; k++) want *= 2u;  // unsigned: wraps, as the shift drops the high bits
      if ((uint64_t)qcode_value(c) != want) bad("qcode_value (shift modulo 64)", c, (uint64_t)qcode_value(c), want);
    }
  }
  for (int64_t v = -4096; v <= 4096; v++) check_v(v);
  for (int k = 1; k <= 62; k++) {
    const int64_t p = (int64_t)1 << k;
    for (int64_t d = -1; d <= 1; d++) {
      check_v(p + d);
      check_v(-(p + d));
    }
  }
  check_v(INT64_MIN);
  check_v(INT64_MAX);
  // 10^6 seeded random 63-bit values (splitmix64), at every magnitude: the
  // low bits of a draw choose how far it is shifted down
  uint64_t st = 0x5EED0900ull;
  for (int i = 0; i < 1000000; i++) {
    st += 0x9E3779B97F4A7C15ull;
    uint64_t z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const uint64_t v63 = z >> 1;
    check_v((int64_t)v63);
    check_v((int64_t)(v63 >> (z & 63u) % 53u));
  }
  if (n_bad) {
    fprintf(stderr, "%llu of %llu checks failed\n", (unsigned long long)n_bad, (unsigned long long)n_checked);
    return 1;
  }
  printf("ok %llu\n", (unsigned long long)n_checked);
  return 0;
}
