// Ranks of the pairs i < j < s in lexicographic order (the order of
// itertools.combinations(range(s), 2)) and their inverse, in 64-bit integer
// arithmetic: the exhaustive miner (das_mine_combinations, miner.hip) maps a
// global rank to a pair of one basic's partner list with it.  Host and device
// (no HIP headers: tests/native/mx_unrank_check.cpp builds it with plain g++).
//
// s < 2^32, so a triangle holds fewer than 2^63 pairs.  Row i starts at
// f(i) = i (2s - i - 1) / 2 and has s - 1 - i pairs.  Counted from the end the
// triangle is the plain one: r' = T - 1 - r lies in the row q with
// q (q + 1) / 2 <= r' < (q + 1)(q + 2) / 2, which is row i = s - 2 - q, and
// j = s - 1 - (r' - q (q + 1) / 2).  q is seeded by a floating sqrt -- wrong
// by more than one above 2^53 -- and decided by the integer comparisons.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DAS_MX_HD __host__ __device__ inline
#else
#define DAS_MX_HD inline
#endif

namespace das {

// pairs of s items
DAS_MX_HD uint64_t mx_pairs(uint64_t s) { return (s & 1) ? s * ((s - 1) >> 1) : (s >> 1) * (s - 1); }

// rank of (i, j), i < j < s
DAS_MX_HD uint64_t mx_rank(uint64_t i, uint64_t j, uint64_t s) {
  const uint64_t w = 2 * s - i - 1;                    // i * w is even: halve the even factor first
  return ((i & 1) ? i * (w >> 1) : (i >> 1) * w) + (j - i - 1);
}

// q (q + 1) / 2 for q < 2^32
DAS_MX_HD uint64_t mx_tri(uint64_t q) { return (q & 1) ? q * ((q + 1) >> 1) : (q >> 1) * (q + 1); }

// the pair of rank r < mx_pairs(s), 2 <= s < 2^32
DAS_MX_HD void mx_unrank(uint64_t r, uint64_t s, uint32_t& i, uint32_t& j) {
  const uint64_t rr = mx_pairs(s) - 1 - r;
  const double seed = __builtin_sqrt(2.0 * (double)rr);
  uint64_t q = seed >= (double)(s - 2) ? s - 2 : (uint64_t)seed;
  while (mx_tri(q) > rr) --q;                          // the correction: q is the last row start <= rr
  while (q < s - 2 && mx_tri(q + 1) <= rr) ++q;
  i = (uint32_t)(s - 2 - q);
  j = (uint32_t)(s - 1 - (rr - mx_tri(q)));
}

}  // namespace das
