// Host check of das_group_counts' rules (das_amd/csrc/group_plan.h) under the
// sanitizers: the strategy choice, the wave's run combining with weights and
// the compaction, on plain arrays against a std::map.  Built by
// `make -C das_amd/csrc group_asan` with -fsanitize=address,undefined; exits
// non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

#include "../das_amd/csrc/group_plan.h"

using namespace das;

static int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

// rows (key, weight) through waves of 64 lanes into bins over [lo, lo + range), then compacted
static void run_case(std::mt19937_64& rng, uint32_t lo, uint32_t range, size_t rows, int shape) {
  std::vector<uint32_t> key(rows);
  std::vector<uint64_t> w(rows);
  for (size_t i = 0; i < rows; ++i) {
    switch (shape) {
      case 0: key[i] = lo + (uint32_t)(rng() % range); break;                      // scattered
      case 1: key[i] = lo + (uint32_t)((uint64_t)i * range / rows); break;         // sorted runs
      case 2: key[i] = lo + range - 1; break;                                      // one key holds every row
      default: key[i] = i % 3 ? lo : lo + (uint32_t)(rng() % range); break;        // a hub between others
    }
    // weights: 1, a product's factor rows (counts pass 2^32), a probe row's count (0 included)
    w[i] = shape == 2 ? 70000ull * 70000ull / rows + 1 : shape == 1 ? rng() % 4 : 1;
  }
  std::map<uint32_t, uint64_t> want;
  for (size_t i = 0; i < rows; ++i)
    if (w[i]) want[key[i]] += w[i];
  std::vector<uint64_t> bins(range, 0);
  unsigned adds = 0;
  for (size_t base = 0; base < rows; base += 64) {
    uint32_t d[64];
    uint64_t ww[64];
    for (int l = 0; l < 64; ++l) {
      const bool in = base + l < rows;
      d[l] = in ? key[base + l] - lo : 0xFFFFFFFFu;
      ww[l] = in ? w[base + l] : 0;
    }
    adds += group_wave_model(d, ww, bins);
  }
  std::vector<uint32_t> ids;
  std::vector<uint64_t> counts;
  const uint64_t n = group_compact_model(bins, lo, ids, counts);
  EXPECT(n == want.size());
  size_t k = 0;
  for (const auto& kv : want) {
    if (k >= ids.size()) break;
    EXPECT(ids[k] == kv.first && counts[k] == kv.second);
    ++k;
  }
  EXPECT(adds <= rows);
  if (shape == 2 && rows) EXPECT(adds == (rows + 63) / 64);                        // one add per wave
}

int main() {
  // the rule
  EXPECT(group_plan(1, 1, 0) == GROUP_DIRECT);
  EXPECT(group_plan(kGroupDirectBins, 1ull << 30, 0) == GROUP_DIRECT);
  EXPECT(group_plan(kGroupDirectBins + 1, kGroupFewRows + 1, 0) == GROUP_SORTED);
  EXPECT(group_plan(kGroupFewRowsBins, kGroupFewRows, 0) == GROUP_DIRECT);          // few rows: a wider range
  EXPECT(group_plan(kGroupFewRowsBins + 1, kGroupFewRows, 0) == GROUP_SORTED);
  EXPECT(group_plan(kGroupMaxBins + 1, kGroupMaxBins, 0) == GROUP_SORTED);
  EXPECT(group_plan(1ull << 32, 10, 0) == GROUP_SORTED);
  EXPECT(group_plan(1ull << 20, 1ull << 33, 0) == GROUP_DIRECT);                    // beyond the sort's rows
  EXPECT(group_plan(1ull << 32, 1ull << 33, 0) == GROUP_NONE);
  // the switches
  EXPECT(group_plan(16, 1000, '0') == GROUP_SORTED);
  EXPECT(group_plan(16, 1ull << 33, '0') == GROUP_DIRECT);                          // the sort's row limit
  EXPECT(group_plan(kGroupMaxBins, 1, '1') == GROUP_DIRECT);
  EXPECT(group_plan(kGroupMaxBins + 1, 1, '1') == GROUP_SORTED);                    // ... wherever memory allows
  EXPECT(kGroupLdsBins * sizeof(uint64_t) <= 64 * 1024);

  std::mt19937_64 rng(20240607);
  const uint32_t ranges[] = {1, 2, 63, 64, 65, kGroupLdsBins - 1, kGroupLdsBins, kGroupLdsBins + 1};
  const size_t rows[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4097};
  for (uint32_t range : ranges)
    for (size_t n : rows)
      for (int shape = 0; shape < 4; ++shape) {
        run_case(rng, 0, range, n, shape);
        run_case(rng, 0xFFFFFFFFu - range + 1, range, n, shape);                    // ids up to 2^32 - 1
      }
  if (fails) {
    std::fprintf(stderr, "group_check: %d mismatches\n", fails);
    return 1;
  }
  std::puts("group_check: ok");
  return 0;
}
