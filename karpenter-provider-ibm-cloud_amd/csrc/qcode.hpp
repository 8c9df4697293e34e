// qcode.hpp — the monotone 16-bit code of a non-negative quantity, for host
// and device: exact below 1024, then a 9-bit mantissa per binade (relative
// step <= 2^-9).  Codes are consecutive in value order, so floor and ceil
// differ by at most one.
//
// With b the bit length of x and s = max(b, 10) - 10, the code of x is
// 512 s + (x >> s): below 1024 that is x itself (s = 0), above it the binade
// index times 512 plus the mantissa's low nine bits (x >> s is in
// [512, 1024)).  Written with selects, no early return: the solver wave runs
// these per placed pod, and a branch on a lane value is an exec-mask section.
// Every shift count stays in 0..63 whatever the input (tests/qcode_check.cpp
// runs every case under the undefined-behaviour sanitizer).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_QCODE_FN __host__ __device__ __forceinline__
#else
#define GS_QCODE_FN static inline
#endif

// binade shift of x: 0 up to 10 bits, bit length - 10 above (<= 54)
GS_QCODE_FN uint32_t qcode_shift(uint64_t x) {
  const uint32_t b = 64u - (uint32_t)__builtin_clzll((unsigned long long)(x | 1ull));
  return (b > 10u ? b : 10u) - 10u;
}

GS_QCODE_FN uint32_t qcode_floor(int64_t v) {
  const uint64_t x = v > 0 ? (uint64_t)v : 0ull;
  const uint32_t s = qcode_shift(x);
  return 512u * s + (uint32_t)(x >> s);
}

GS_QCODE_FN uint32_t qcode_ceil(int64_t v) {
  const uint64_t x = v > 0 ? (uint64_t)v : 0ull;
  const uint32_t s = qcode_shift(x);
  return 512u * s + (uint32_t)(x >> s) + ((x & ((1ull << s) - 1ull)) ? 1u : 0u);
}

// the value a code stands for: qcode_floor(v) <= v's code <= qcode_ceil(v)
// and qcode_value(qcode_floor(v)) <= v <= qcode_value(qcode_ceil(v)).
// (No quantity has a code of 33,280 or more, where the binade shift would
// pass 63; the count is taken modulo 64 there, as the shifters do.)
GS_QCODE_FN int64_t qcode_value(uint32_t c) {
  const bool big = c >= 1024u;
  const uint32_t s = big ? (c >> 9) - 1u : 0u;
  const uint32_t m = big ? (c & 511u) + 512u : c;
  return (int64_t)((uint64_t)m << (s & 63u));
}
