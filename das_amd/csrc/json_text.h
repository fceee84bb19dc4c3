// JSON string text as Python's json.dumps(..., ensure_ascii=True) writes it:
// the per-code-point rules of the atom documents (docs.hip), in one place.
// Host and device compile this header (tests/native/json_text_check.cpp runs
// it with plain g++), so the measured length and the written bytes of a name
// come from the same code.
//
//   "  -> \"      \  -> \\      \n \r \t \b \f -> the two-character forms
//   any other byte < 0x20, and 0x7f  -> \u00xx (lower-case hex)
//   printable ASCII as it is ('/' too)
//   U+0080 .. U+FFFF -> \uxxxx;  above: the surrogate pair (U+10000 -> 𐀀)
//
// Input is UTF-8.  Overlong forms, encoded surrogates, code points above
// U+10FFFF, stray continuation bytes and truncated sequences are malformed:
// each such byte is consumed alone, counted, and stands as U+FFFD in the text
// (so length and write still agree; the caller discards a text with a count).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DAS_JT_HD __host__ __device__ inline
#else
#define DAS_JT_HD inline
#endif

namespace das {

constexpr uint32_t kJtMaxEscape = 12;    // bytes one code point becomes at most (a surrogate pair)
constexpr uint32_t kJtReplacement = 0xFFFDu;

struct JtCodePoint {
  uint32_t cp;      // the code point (kJtReplacement where malformed)
  uint32_t used;    // input bytes consumed (>= 1)
  uint32_t bad;     // 1: malformed at this byte
};

// The code point that begins at byte i of the `len` bytes get(0 .. len - 1); i < len.
template <typename Get>
DAS_JT_HD JtCodePoint jt_decode(Get get, uint64_t i, uint64_t len) {
  const uint32_t b0 = get(i);
  if (b0 < 0x80u) return JtCodePoint{b0, 1, 0};
  uint32_t need, cp, min_cp;
  if (b0 >= 0xC2u && b0 <= 0xDFu) { need = 1; cp = b0 & 0x1Fu; min_cp = 0x80u; }
  else if (b0 >= 0xE0u && b0 <= 0xEFu) { need = 2; cp = b0 & 0x0Fu; min_cp = 0x800u; }
  else if (b0 >= 0xF0u && b0 <= 0xF4u) { need = 3; cp = b0 & 0x07u; min_cp = 0x10000u; }
  else return JtCodePoint{kJtReplacement, 1, 1};              // a continuation byte, C0 / C1, F5 .. FF
  if (len - i <= need) return JtCodePoint{kJtReplacement, 1, 1};   // truncated
  for (uint32_t k = 1; k <= need; ++k) {
    const uint32_t b = get(i + k);
    if ((b & 0xC0u) != 0x80u) return JtCodePoint{kJtReplacement, 1, 1};
    cp = (cp << 6) | (b & 0x3Fu);
  }
  if (cp < min_cp || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) return JtCodePoint{kJtReplacement, 1, 1};
  return JtCodePoint{cp, need + 1, 0};
}

DAS_JT_HD uint32_t jt_escaped_len_cp(uint32_t cp) {
  if (cp >= 0x10000u) return 12;
  if (cp >= 0x7Fu) return 6;
  if (cp >= 0x20u) return (cp == 0x22u || cp == 0x5Cu) ? 2 : 1;
  return (cp == 0x0Au || cp == 0x0Du || cp == 0x09u || cp == 0x08u || cp == 0x0Cu) ? 2 : 6;
}

DAS_JT_HD uint8_t jt_hex(uint32_t v) { return (uint8_t)(v < 10 ? '0' + v : 'a' + (v - 10)); }

DAS_JT_HD void jt_u16(uint32_t v, uint8_t* buf) {
  buf[0] = '\\';
  buf[1] = 'u';
  buf[2] = jt_hex((v >> 12) & 15u);
  buf[3] = jt_hex((v >> 8) & 15u);
  buf[4] = jt_hex((v >> 4) & 15u);
  buf[5] = jt_hex(v & 15u);
}

// The escaped form of one code point into buf[0 .. kJtMaxEscape): its length
// (= jt_escaped_len_cp(cp)).
DAS_JT_HD uint32_t jt_escape_cp(uint32_t cp, uint8_t* buf) {
  if (cp >= 0x10000u) {
    const uint32_t v = cp - 0x10000u;
    jt_u16(0xD800u | (v >> 10), buf);
    jt_u16(0xDC00u | (v & 0x3FFu), buf + 6);
    return 12;
  }
  uint8_t two = 0;
  switch (cp) {
    case 0x22u: two = '"'; break;
    case 0x5Cu: two = '\\'; break;
    case 0x0Au: two = 'n'; break;
    case 0x0Du: two = 'r'; break;
    case 0x09u: two = 't'; break;
    case 0x08u: two = 'b'; break;
    case 0x0Cu: two = 'f'; break;
    default: break;
  }
  if (two) {
    buf[0] = '\\';
    buf[1] = two;
    return 2;
  }
  if (cp >= 0x20u && cp < 0x7Fu) {
    buf[0] = (uint8_t)cp;
    return 1;
  }
  jt_u16(cp, buf);
  return 6;
}

// Bytes of the escaped text of the `len` bytes get(0 ..); *n_bad += the malformed bytes.
template <typename Get>
DAS_JT_HD uint64_t jt_escaped_len(Get get, uint64_t len, uint32_t* n_bad) {
  uint64_t out = 0;
  uint32_t bad = 0;
  for (uint64_t i = 0; i < len;) {
    const JtCodePoint c = jt_decode(get, i, len);
    out += jt_escaped_len_cp(c.cp);
    bad += c.bad;
    i += c.used;
  }
  if (n_bad) *n_bad += bad;
  return out;
}

// The escaped text, byte by byte through put(position, byte), positions
// ascending from `at`: the position after the last byte (at + jt_escaped_len).
template <typename Get, typename Put>
DAS_JT_HD uint64_t jt_escape(Get get, uint64_t len, Put put, uint64_t at) {
  uint8_t buf[kJtMaxEscape];
  for (uint64_t i = 0; i < len;) {
    const JtCodePoint c = jt_decode(get, i, len);
    const uint32_t n = jt_escape_cp(c.cp, buf);
    for (uint32_t k = 0; k < n; ++k) put(at + k, buf[k]);
    at += n;
    i += c.used;
  }
  return at;
}

}  // namespace das
