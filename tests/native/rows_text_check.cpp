// Host check of das_amd/csrc/rows_text.h (das_table_rows_text's size, tile and
// hex rules), compiled by tests/test_query_text.py with plain g++ and with
// -fsanitize=address,undefined.  Everything is checked against the obvious
// slow form:
//   hex     rt_hex8 against "%02x" per byte: every value of each 16-bit half,
//           digests with leading-zero bytes
//   tiles   for every unit (a row and its separator) up to the limit: the
//           rows per tile fill the stage with room for any start residue mod
//           16, one more row would not fit, and the tiles' spans are
//           consecutive, begin at 0 and end at the total
//   bytes   for small units, every window size around the tile's row count
//           and every cap of interest: the kernel's write phase (whole
//           16-byte vectors, edge bytes) replayed on a byte map covers every
//           byte of [0, min(total, cap)) exactly once and none outside
//   product rt_product_row against / and %
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../das_amd/csrc/rows_text.h"

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "FAILED %s: ", #cond);          \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      std::exit(1);                                        \
    }                                                      \
  } while (0)

using namespace das;

static void hex_slow(const uint8_t* bytes, int n, char* out) {
  for (int i = 0; i < n; ++i) std::snprintf(out + 2 * i, 3, "%02x", bytes[i]);
}

static void check_word(uint32_t w) {
  uint8_t b[4];
  std::memcpy(b, &w, 4);
  char want[9], got[9] = {0};
  hex_slow(b, 4, want);
  const uint64_t x = rt_hex8(w);
  std::memcpy(got, &x, 8);
  CHECK(std::memcmp(want, got, 8) == 0, "word %08x: %s, expected %s", w, got, want);
}

static void check_hex() {
  for (uint32_t v = 0; v < 65536; ++v) {
    check_word(v);
    check_word(v << 16);
    check_word(v * 0x00010001u);
    check_word(v ^ 0xA5C30F69u);
  }
  // whole digests, leading-zero bytes included: 32 characters in memory order
  const uint8_t digests[][16] = {
      {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {0, 0, 0, 1, 0x0a, 0xa0, 0x09, 0x90, 0xff, 0, 0xf0, 0x0f, 0x9a, 0xa9, 0, 0x10},
      {0xaf, 0x12, 0xf1, 0x0f, 0x9a, 0xe2, 0x00, 0x2a, 0x16, 0x07, 0xba, 0x0b, 0x47, 0xba, 0x84, 0x07},
      {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff},
  };
  for (const auto& d : digests) {
    char want[33], got[33] = {0};
    hex_slow(d, 16, want);
    for (int k = 0; k < 4; ++k) {
      uint32_t w;
      std::memcpy(&w, d + 4 * k, 4);
      const uint64_t x = rt_hex8(w);
      std::memcpy(got + 8 * k, &x, 8);
    }
    CHECK(std::memcmp(want, got, 32) == 0, "digest: %s, expected %s", got, want);
  }
}

static void check_tiles() {
  CHECK(rt_rows_per_tile(0) == 0 && rt_rows_per_tile(kRtMaxUnit + 1) == 0, "limits");
  CHECK(rt_total(0, 40, 2) == 0 && rt_total(1, 40, 2) == 38 && rt_total(3, 40, 2) == 118, "totals");
  for (uint64_t unit = 1; unit <= kRtMaxUnit; ++unit) {
    const uint32_t T = rt_rows_per_tile(unit);
    CHECK(T >= 1, "unit %llu: no row fits", (unsigned long long)unit);
    // any start residue: the image of T rows (the last row's separator too) fits the stage
    for (uint32_t shift = 0; shift < 16; ++shift)
      CHECK(shift + (uint64_t)T * unit <= kRtStage, "unit %llu: image beyond the stage", (unsigned long long)unit);
    CHECK(15 + (uint64_t)(T + 1) * unit > kRtStage - 1, "unit %llu: a further row fits", (unsigned long long)unit);
    // a row holds a handle at least: the separator is what is left of the unit at most
    const uint64_t seps[] = {0, 1, 2, 17};
    for (uint64_t sep : seps) {
      if (unit < kRtHex + sep) continue;
      const uint64_t nrows = 17ull * T + 1;                 // 18 tiles, the last of one row
      const uint64_t total = rt_total(nrows, unit, sep), tiles = rt_tiles(nrows, T);
      CHECK(tiles == 18, "unit %llu: %llu tiles", (unsigned long long)unit, (unsigned long long)tiles);
      uint64_t at = 0, rows = 0;
      for (uint64_t k = 0; k < tiles; ++k) {
        const RtTile t = rt_tile(k, nrows, unit, sep, T);
        CHECK(t.begin == at && t.row0 == rows && t.rows >= 1 && t.rows <= T, "unit %llu tile %llu: not consecutive",
              (unsigned long long)unit, (unsigned long long)k);
        CHECK(t.base % 16 == 0 && t.base <= t.begin && t.begin - t.base < 16, "unit %llu: base", (unsigned long long)unit);
        CHECK(t.end > t.begin && t.end <= total, "unit %llu: span outside the text", (unsigned long long)unit);
        CHECK(t.end - t.base <= kRtStage, "unit %llu: span beyond the image", (unsigned long long)unit);
        at = t.end;
        rows += t.rows;
      }
      CHECK(at == total && rows == nrows, "unit %llu: the tiles do not end at the total", (unsigned long long)unit);
    }
  }
}

// the kernel's write phase on a byte map
static void replay(uint64_t nrows, uint64_t unit, uint64_t sep, uint64_t cap) {
  const uint32_t T = rt_rows_per_tile(unit);
  const uint64_t total = rt_total(nrows, unit, sep);
  const uint64_t k = total < cap ? total : cap;
  std::vector<uint8_t> hits(total + 64, 0);
  for (uint64_t tile = 0; tile < rt_tiles(nrows, T); ++tile) {
    const RtTile t = rt_tile(tile, nrows, unit, sep, T);
    const uint64_t te = t.end < k ? t.end : k;
    if (t.begin >= te) break;
    const uint64_t nvec = (te - t.base + 15) >> 4;
    for (uint64_t v = 0; v < nvec; ++v) {
      const uint64_t g = t.base + 16 * v;
      CHECK(16 * v + 16 <= kRtStage, "vector beyond the image");
      if (rt_vec_whole(g, t.begin, te)) {
        for (int b = 0; b < 16; ++b) hits[g + b]++;
      } else {
        const uint64_t e0 = g > t.begin ? g : t.begin, e1 = g + 16 < te ? g + 16 : te;
        for (uint64_t p = e0; p < e1; ++p) hits[p]++;
      }
    }
  }
  for (uint64_t p = 0; p < hits.size(); ++p)
    CHECK(hits[p] == (p < k ? 1 : 0), "nrows %llu unit %llu sep %llu cap %llu: byte %llu written %d times",
          (unsigned long long)nrows, (unsigned long long)unit, (unsigned long long)sep, (unsigned long long)cap,
          (unsigned long long)p, (int)hits[p]);
}

static void check_bytes() {
  std::vector<uint64_t> units;
  for (uint64_t u = 32; u <= 80; ++u) units.push_back(u);   // every residue mod 16, three times over
  for (uint64_t u : {63ull, 64ull, 65ull, 86ull, 127ull, 128ull, 129ull, 1023ull, 1024ull, 1025ull, 8183ull, 8184ull, 8185ull, (unsigned long long)kRtMaxUnit - 1,
                     (unsigned long long)kRtMaxUnit})
    units.push_back(u);
  for (uint64_t unit : units) {
    const uint32_t T = rt_rows_per_tile(unit);
    const uint64_t seps[] = {0, 2};
    for (uint64_t sep : seps) {
      if (unit < kRtHex + sep) continue;
      const uint64_t ns[] = {1, T - 1ull, T, T + 1ull, 2ull * T + 1};
      for (uint64_t nrows : ns) {
        if (!nrows) continue;
        const uint64_t total = rt_total(nrows, unit, sep);
        const uint64_t caps[] = {0, 1, 15, 16, 17, total ? total - 1 : 0, total, total + 5};
        for (uint64_t cap : caps) replay(nrows, unit, sep, cap);
      }
    }
  }
}

static void check_product() {
  const uint64_t nbs[] = {1, 2, 3, 7, 69, 70, 71, 255, 256, 511, 512, 32767, 32768, 32769, 70000,
                          (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, 1ull << 40};
  for (uint64_t nb : nbs) {
    const uint64_t b0s[] = {0, nb / 2, nb - 1};
    for (uint64_t b0 : b0s) {
      for (uint64_t p0 : {0ull, 5ull, 1ull << 33}) {
        for (uint32_t r = 0; r < 32768; r += (r < 1024 ? 1 : 127)) {
          uint64_t p, b;
          rt_product_row(p0, b0, r, nb, &p, &b);
          CHECK(p == p0 + (b0 + r) / nb && b == (b0 + r) % nb, "nb %llu b0 %llu r %u", (unsigned long long)nb, (unsigned long long)b0, r);
        }
      }
    }
  }
}

int main() {
  check_hex();
  check_tiles();
  check_bytes();
  check_product();
  std::printf("ok stage %u max_row %u\n", kRtStage, kRtMaxUnit);
  return 0;
}
