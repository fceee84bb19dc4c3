// The text of ordered rows (das_table_rows_text, rows_text.hip): every row is
// the same literals around 32-character holes, so sizes and positions are
// closed forms.  Host and device compile this header
// (tests/native/rows_text_check.cpp runs it with plain g++), so the size the
// host reports, the tiles it launches and the bytes a tile writes come from
// the same code.
//
//   unit  = R + sep_len: a row's text and the separator after it
//   total = nrows * unit - sep_len (the last row has no separator; 0 rows: 0)
//   row i of the window begins at byte i * unit
//   tile k = rows [k * T, min((k + 1) * T, nrows)), bytes [k * T * unit,
//            min((k + 1) * T * unit, total)): consecutive rows, one span
//   the tile's image begins at the 16-byte boundary at or below its span's
//   first byte, so T * unit + 15 bytes fit the stage
#pragma once
#include <cstdint>

#include "../../include/das_mi355x.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DAS_RT_HD __host__ __device__ inline
#else
#define DAS_RT_HD inline
#endif

namespace das {

constexpr uint32_t kRtStage = DAS_ROWS_TEXT_STAGE_BYTES;   // bytes of a tile's image
constexpr uint32_t kRtMaxUnit = DAS_ROWS_TEXT_MAX_ROW;     // R + sep_len at most
constexpr uint32_t kRtHex = 32;                            // characters of a handle
static_assert(kRtStage % 16 == 0 && kRtMaxUnit + 16 <= kRtStage, "a row and its alignment slack fit the stage");

// Rows of a tile for rows of `unit` bytes (separator included); 0: beyond the limit.
DAS_RT_HD uint32_t rt_rows_per_tile(uint64_t unit) {
  return unit == 0 || unit > kRtMaxUnit ? 0u : (uint32_t)((kRtStage - 16) / unit);
}

DAS_RT_HD uint64_t rt_total(uint64_t nrows, uint64_t unit, uint64_t sep_len) {
  return nrows ? nrows * unit - sep_len : 0;
}

DAS_RT_HD uint64_t rt_tiles(uint64_t nrows, uint32_t rows_per_tile) {
  return (nrows + rows_per_tile - 1) / rows_per_tile;
}

struct RtTile {
  uint64_t row0;     // first row of the window in the tile
  uint32_t rows;     // its rows (>= 1)
  uint64_t begin;    // output bytes [begin, end)
  uint64_t end;
  uint64_t base;     // begin rounded down to 16: output byte p is image byte p - base
};

// Tile k < rt_tiles(nrows, T) of a window of nrows rows.
DAS_RT_HD RtTile rt_tile(uint64_t k, uint64_t nrows, uint64_t unit, uint64_t sep_len, uint32_t T) {
  RtTile t;
  t.row0 = k * T;
  const uint64_t left = nrows - t.row0;
  t.rows = left < T ? (uint32_t)left : T;
  t.begin = t.row0 * unit;
  t.end = t.row0 + t.rows == nrows ? rt_total(nrows, unit, sep_len) : t.begin + (uint64_t)t.rows * unit;
  t.base = t.begin & ~15ull;
  return t;
}

// Whether the 16 output bytes at g (a multiple of 16) of a tile writing
// [begin, te) leave as one vector; otherwise its bytes inside [begin, te) go
// one by one (the rest are a neighbour tile's, or at or past the cap).
DAS_RT_HD bool rt_vec_whole(uint64_t g, uint64_t begin, uint64_t te) { return g >= begin && g + 16 <= te; }

// The 8 lower-case hex characters of the 4 bytes of `w` in memory order
// (little-endian word in, little-endian characters out): byte 0's high
// nibble is the first character.
DAS_RT_HD uint64_t rt_hex8(uint32_t w) {
  uint64_t x = w;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;                      // byte i at character 2i
  const uint64_t n = ((x >> 4) & 0x000F000F000F000Full) | ((x & 0x000F000F000F000Full) << 8);
  const uint64_t af = ((n + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;   // 1 where the nibble is a .. f
  return n + 0x3030303030303030ull + af * 39u;                     // '0' + n, 'a' - 10 + n
}

// Output row o0 + r of a deferred product of nb build rows, where (p0, b0) =
// (o0 / nb, o0 % nb) and r < 2^15: its probe and build rows, without a 64-bit
// division.
DAS_RT_HD void rt_product_row(uint64_t p0, uint64_t b0, uint32_t r, uint64_t nb, uint64_t* p, uint64_t* b) {
  uint64_t x = b0 + r;
  if (x >= nb) {
    if (nb >> 15) {            // r < 2^15 <= nb: one wrap at most
      x -= nb;
      p0 += 1;
    } else {                   // x < 2^16
      const uint32_t q = (uint32_t)x / (uint32_t)nb;
      x = (uint32_t)x - q * (uint32_t)nb;
      p0 += q;
    }
  }
  *p = p0;
  *b = x;
}

}  // namespace das
