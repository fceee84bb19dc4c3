// Host-side rules of das_group_counts (group.hip), free of device code so that
// tools/group_check.cpp exercises them under the sanitizers: the constants, the
// choice of a counting strategy, and a plain-array model of the weighting, the
// wave's run combining and the compaction.
#pragma once
#include <cstdint>
#include <vector>

namespace das {

// 64-bit bins of the LDS tile (32 KiB of the CU's 160 KiB: five workgroups
// resident).  Measured at the tile's edge (profiles/group_counts.json, 2^22
// rows of uniform keys): 4096 bins in LDS 0.18 ms, 4097 bins through global
// atomics 0.32 ms; no difference at 4096 rows.  A larger tile is unmeasured.
constexpr uint32_t kGroupLdsBins = 4096;
// rows a workgroup of the LDS kernel takes at least (it flushes up to
// kGroupLdsBins adds: at most one flushed add per four rows read)
constexpr uint64_t kGroupLdsRows = 4ull * kGroupLdsBins;
// Direct counters whatever the row count up to this range.  Measured (same
// file, two runs on two boxes): 2^22 rows of uniform keys take 0.36 ms directly
// against 0.50 ms sorted at 2^16 bins in both; at 2^20 bins and more the direct
// form took 1.1 - 4.4 ms in one run, level with the sort, and 30 ms in the
// other (cause not found), the sort 1.4 - 4.0 ms in both.  Ranges between 2^16
// and 2^20 are unmeasured and take the sort.
constexpr uint64_t kGroupDirectBins = 1ull << 16;
// ... and for few rows up to a wider range: 4096 rows take 0.12 ms directly
// against 0.17 ms sorted at 2^22 bins, 0.18 against 0.17 ms at 2^24 and 0.54
// against 0.19 ms at 2^26 (zeroing and scanning the bins); the row limit is
// where 0.09 ms + 7.1 ns per scattered add meets the sort's 0.15 ms + 0.8 ns
// per row (about 9500 rows).
constexpr uint64_t kGroupFewRows = 8192;
constexpr uint64_t kGroupFewRowsBins = 1ull << 22;
// no direct counters beyond this range (768 MiB of counters and offsets)
constexpr uint64_t kGroupMaxBins = 1ull << 26;
// the sort's row limit (radix_sort_pairs)
constexpr uint64_t kGroupMaxSortRows = (1ull << 32) - 1;

enum GroupPlan { GROUP_NONE = 0, GROUP_DIRECT = 1, GROUP_SORTED = 2 };

// `force`: DAS_GROUP_DIRECT's first character ('0' sorted everywhere, '1'
// direct wherever memory allows, else the rule)
inline GroupPlan group_plan(uint64_t range, uint64_t rows, char force) {
  const bool can_direct = range <= kGroupMaxBins, can_sort = rows <= kGroupMaxSortRows;
  bool direct = range <= kGroupDirectBins || (rows <= kGroupFewRows && range <= kGroupFewRowsBins);
  if (force == '0') direct = false;
  if (force == '1') direct = true;
  if (direct && can_direct) return GROUP_DIRECT;
  if (can_sort) return GROUP_SORTED;
  return can_direct ? GROUP_DIRECT : GROUP_NONE;
}

// One wave's step of the accumulate kernels on plain arrays: 64 lanes of
// (bin, weight), bin 0xFFFFFFFF = no row; a run of equal bins in consecutive
// lanes is added once, by its first lane, with the run's weight sum taken from
// the wave's inclusive scan.  Returns the adds issued.
inline unsigned group_wave_model(const uint32_t d[64], const uint64_t w[64], std::vector<uint64_t>& bins) {
  uint64_t heads = 0, incl[64], acc = 0;
  for (int l = 0; l < 64; ++l) {
    if (l == 0 || d[l - 1] != d[l]) heads |= 1ull << l;
    incl[l] = acc += w[l];
  }
  unsigned adds = 0;
  for (int l = 0; l < 64; ++l) {
    if (!((heads >> l) & 1)) continue;
    uint64_t sum = w[l];
    if (heads != ~0ull) {
      const uint64_t above = l == 63 ? 0ull : heads >> (l + 1);
      const int last = above ? l + __builtin_ffsll((long long)above) - 1 : 63;
      sum = incl[last] - (incl[l] - w[l]);
    }
    if (d[l] != 0xFFFFFFFFu && sum) {
      bins.at(d[l]) += sum;
      ++adds;
    }
  }
  return adds;
}

// The compaction on plain arrays: non-zero bins to (lo + bin, count) at the
// exclusive prefix of the non-zero flags.
inline uint64_t group_compact_model(const std::vector<uint64_t>& bins, uint32_t lo, std::vector<uint32_t>& ids,
                                    std::vector<uint64_t>& counts) {
  std::vector<uint32_t> off(bins.size() + 1, 0);
  for (size_t i = 0; i < bins.size(); ++i) off[i + 1] = off[i] + (bins[i] ? 1u : 0u);
  ids.assign(off.back(), 0);
  counts.assign(off.back(), 0);
  for (size_t i = 0; i < bins.size(); ++i)
    if (bins[i]) {
      ids.at(off[i]) = lo + (uint32_t)i;
      counts.at(off[i]) = bins[i];
    }
  return off.back();
}

}  // namespace das
