// Host check of das_amd/csrc/mx_unrank.h (built and run by tests/test_mine.py):
// unrank(rank(i, j, s), s) == (i, j) for every pair of the small triangles and
// at the first and last rank of every row of the large ones, whose ranks pass
// 2^53 (where a double no longer holds them).  The rows of a large triangle
// are split over up to 16 threads.  Prints "ok <pairs checked>".
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../das_amd/csrc/mx_unrank.h"

static std::atomic<unsigned long long> checked{0};
static std::atomic<int> failed{0};

static bool check(uint64_t i, uint64_t j, uint64_t s) {
  const uint64_t r = das::mx_rank(i, j, s);
  uint32_t gi = 0, gj = 0;
  das::mx_unrank(r, s, gi, gj);
  if (r < das::mx_pairs(s) && gi == i && gj == j) return true;
  if (!failed.exchange(1))
    std::printf("FAIL s=%llu (%llu,%llu) rank %llu -> (%u,%u)\n", (unsigned long long)s, (unsigned long long)i,
                (unsigned long long)j, (unsigned long long)r, gi, gj);
  return false;
}

// first and last pair of the rows [a, b) of the triangle of s
static void rows(uint64_t a, uint64_t b, uint64_t s) {
  unsigned long long n = 0;
  for (uint64_t i = a; i < b && !failed.load(std::memory_order_relaxed); ++i) {
    if (!check(i, i + 1, s) || !check(i, s - 1, s)) return;
    n += 2;
  }
  checked += n;
}

int main() {
  const uint64_t small[] = {2, 3, 4, 65, 1000};
  for (uint64_t s : small) {
    uint64_t want = 0;                                  // ranks run 0, 1, .. in lexicographic order
    for (uint64_t i = 0; i + 1 < s; ++i)
      for (uint64_t j = i + 1; j < s; ++j) {
        if (das::mx_rank(i, j, s) != want++) {
          std::printf("FAIL rank order s=%llu\n", (unsigned long long)s);
          return 1;
        }
        if (!check(i, j, s)) return 1;
        ++checked;
      }
    if (want != das::mx_pairs(s)) return 1;
  }
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const uint64_t large[] = {(1ull << 16) + 1, (1ull << 31) - 1, (1ull << 32) - 1};
  for (uint64_t s : large) {
    const uint64_t nrows = s - 1, per = (nrows + nt - 1) / nt;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
      pool.emplace_back(rows, std::min<uint64_t>(t * per, nrows), std::min<uint64_t>((t + 1) * per, nrows), s);
    for (auto& th : pool) th.join();
    if (failed) return 1;
  }
  // the last triangle's ranks are beyond what a double holds
  if (das::mx_rank((1ull << 32) - 3, (1ull << 32) - 2, (1ull << 32) - 1) < (1ull << 53)) return 1;
  std::printf("ok %llu\n", checked.load());
  return 0;
}
