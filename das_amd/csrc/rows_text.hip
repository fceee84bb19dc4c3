// The rows of an ordered table as text (das_table_rows_text):
// row r is lit[0] hex(col0[r]) lit[1] .. lit[ncols], the rows joined by `sep`.
// Every row has the same length, so nothing is measured or scanned: the host
// knows the size and every row's position (rows_text.h) before the one launch.
//
// A tile is a run of consecutive rows, its output one contiguous span.  The
// workgroup builds the image of that span in LDS from the 16-byte boundary at
// or below the span's first byte of the OUTPUT (the alignment is the absolute
// output offset's, not the tile's): the literal bytes from a host-built
// (position, byte) list, then one 16-byte digest load and 32 hex characters
// per cell.  The image leaves in whole 16-byte nontemporal stores (plain
// stores measured 15 to 35 % slower); the edge vectors a tile
// shares with its neighbour, the window's end or `cap` go byte by byte.
//
// Unresolved answers are read from what they keep: a VIEW's index columns in
// place, a PRODUCT's factor columns (output row o = probe row o / nb, build
// row o % nb; no k_cartesian launch, the table stays deferred); an EXPAND is
// settled first.
#include "das_internal.h"
#include "rows_text.h"

namespace das {
namespace {

constexpr int kRtBlock = 256;
typedef uint32_t rt_v4u __attribute__((ext_vector_type(4)));

struct RowsSrc {
  const uint32_t* col[kMaxCols];   // column c (PRODUCT: of the factor side[c] names)
  uint32_t hole[kMaxCols];         // byte of a row's text where column c's hex begins
  uint8_t side[kMaxCols];          // PRODUCT: 1 = indexed by the build row
  uint64_t nb;                     // PRODUCT: build rows; 0: col[c][row]
  uint64_t row0;                   // the window's first row
  uint32_t ncols;
};

// The 32 hex characters of digest d at image byte a (any alignment): words
// where they are whole, bytes at the two ends (the neighbouring bytes of those
// words are literals other threads write).
__device__ __forceinline__ void put_hex(uint8_t* img, uint32_t a, const uint4& d) {
  uint32_t h[8];
  const uint64_t x0 = rt_hex8(d.x), x1 = rt_hex8(d.y), x2 = rt_hex8(d.z), x3 = rt_hex8(d.w);
  h[0] = (uint32_t)x0; h[1] = (uint32_t)(x0 >> 32);
  h[2] = (uint32_t)x1; h[3] = (uint32_t)(x1 >> 32);
  h[4] = (uint32_t)x2; h[5] = (uint32_t)(x2 >> 32);
  h[6] = (uint32_t)x3; h[7] = (uint32_t)(x3 >> 32);
  const uint32_t m = a & 3u;
  uint32_t* w = reinterpret_cast<uint32_t*>(img + (a - m));
  if (m == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = h[k];
    return;
  }
  const uint32_t sh = 8u * m;
  for (uint32_t i = m; i < 4; ++i) img[a - m + i] = (uint8_t)(h[0] >> (8u * (i - m)));
#pragma unroll
  for (int k = 1; k < 8; ++k) w[k] = __funnelshift_r(h[k - 1], h[k], 32u - sh);
  for (uint32_t i = 0; i < m; ++i) img[a - m + 32u + i] = (uint8_t)(h[7] >> (32u - sh + 8u * i));
}

// out[0 .. min(total, cap)) = the text of rows [src.row0, src.row0 + nrows):
// rows of `unit` bytes (the separator's sep_len included), T rows per tile.
// lit[0 .. L): the literal and separator bytes of one row as position << 8 |
// byte.  `out` is 16-byte aligned; nothing is stored at or past out[cap].
__global__ void __launch_bounds__(kRtBlock) k_rows_text(RowsSrc src, const Digest* __restrict__ digest,
                                                        uint64_t n_atoms, const uint32_t* __restrict__ lit,
                                                        uint32_t L, uint64_t nrows, uint32_t unit, uint32_t sep_len,
                                                        uint32_t T, uint64_t cap, uint8_t* __restrict__ out,
                                                        unsigned long long* n_bad) {
  __shared__ rt_v4u s_img[kRtStage / 16];
  uint8_t* img = reinterpret_cast<uint8_t*>(s_img);
  const uint32_t tid = threadIdx.x;
  const uint64_t tiles = rt_tiles(nrows, T);
  // entry tid, tid + 256, .. of a tile's (row, literal) and (row, column)
  // pairs, stepped without a division
  const uint32_t lq = L ? kRtBlock / L : 0, lr = L ? kRtBlock % L : 0;
  const uint32_t lrow0 = L ? tid / L : 0, lj0 = L ? tid % L : 0;
  const uint32_t cq = kRtBlock / src.ncols, cr = kRtBlock % src.ncols;
  const uint32_t crow0 = tid / src.ncols, cc0 = tid % src.ncols;
  for (uint64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const RtTile t = rt_tile(k, nrows, unit, sep_len, T);
    const uint64_t te = t.end < cap ? t.end : cap;
    if (t.begin >= te) break;                                   // at the cap, as every later tile (block-uniform)
    const uint32_t shift = (uint32_t)(t.begin - t.base);
    __syncthreads();                                            // the previous tile's image was written out
    if (L) {
      uint32_t row = lrow0, j = lj0;
      while (row < t.rows) {
        const uint32_t e = lit[j];
        img[shift + row * unit + (e >> 8)] = (uint8_t)e;
        row += lq;
        j += lr;
        if (j >= L) {
          j -= L;
          ++row;
        }
      }
    }
    uint64_t p0 = 0, b0 = 0;
    if (src.nb) {
      const uint64_t o0 = src.row0 + t.row0;
      p0 = o0 / src.nb;
      b0 = o0 % src.nb;
    }
    {
      uint32_t row = crow0, c = cc0;
      while (row < t.rows) {
        uint64_t pr = src.row0 + t.row0 + row, br = 0;
        if (src.nb) rt_product_row(p0, b0, row, src.nb, &pr, &br);
        const uint32_t id = src.col[c][src.side[c] ? br : pr];
        uint4 d = make_uint4(0, 0, 0, 0);
        if (id < n_atoms) d = *reinterpret_cast<const uint4*>(digest + id);
        else atomicAdd(n_bad, 1ull);
        put_hex(img, shift + row * unit + src.hole[c], d);
        row += cq;
        c += cr;
        if (c >= src.ncols) {
          c -= src.ncols;
          ++row;
        }
      }
    }
    __syncthreads();
    const uint32_t nvec = (uint32_t)((te - t.base + 15) >> 4);
    for (uint32_t v = tid; v < nvec; v += kRtBlock) {
      const uint64_t g = t.base + 16ull * v;
      if (rt_vec_whole(g, t.begin, te)) {
        __builtin_nontemporal_store(s_img[v], reinterpret_cast<rt_v4u*>(out + g));
      } else {                                                  // shared with a neighbour tile, the end or the cap
        const uint64_t e0 = g > t.begin ? g : t.begin, e1 = g + 16 < te ? g + 16 : te;
        for (uint64_t p = e0; p < e1; ++p) out[p] = img[p - t.base];
      }
    }
  }
}

}  // namespace

uint64_t table_rows_text(Ctx& c, Table& t, uint64_t row0, uint64_t nrows, const uint8_t* lit, const uint32_t* lit_off,
                         const uint8_t* sep, uint32_t sep_len, uint8_t* out, uint64_t cap, uint64_t* n_bad) {
  if (t.lazy)
    DAS_CHECK(!t.lazy->aliases_index() || t.lazy->ctx == &c, DAS_E_INVALID,
              "an unresolved answer is read through the context that made it");
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  DAS_CHECK(t.kind == DAS_TABLE_ORDERED, DAS_E_INVALID, "rows text of a table that is not ORDERED");
  DAS_CHECK(t.ncols >= 1, DAS_E_INVALID, "rows text of a table without columns");
  DAS_CHECK(row0 <= t.nrows && nrows <= t.nrows - row0, DAS_E_INVALID, "rows out of range");
  DAS_CHECK(lit_off && (lit || lit_off[t.ncols + 1] == lit_off[0]), DAS_E_INVALID, "null literals");
  DAS_CHECK(sep || !sep_len, DAS_E_INVALID, "null separator");
  DAS_CHECK(out || !cap, DAS_E_INVALID, "null text buffer");
  const uint32_t ncols = (uint32_t)t.ncols;
  for (uint32_t i = 0; i <= ncols; ++i)
    DAS_CHECK(lit_off[i] <= lit_off[i + 1], DAS_E_INVALID, "literal offsets not ascending");
  const uint64_t unit = (uint64_t)(lit_off[ncols + 1] - lit_off[0]) + (uint64_t)kRtHex * ncols + sep_len;
  const uint32_t T = rt_rows_per_tile(unit);
  DAS_CHECK(T, DAS_E_LIMIT, "rows text: a row and its separator exceed DAS_ROWS_TEXT_MAX_ROW bytes");
  if (t.lazy && t.lazy->kind == Lazy::EXPAND) settle(c, t);
  if (n_bad) *n_bad = 0;
  const uint64_t total = rt_total(nrows, unit, sep_len);
  const uint64_t k = std::min(total, cap);
  if (!k) return total;

  RowsSrc src{};
  src.ncols = ncols;
  src.row0 = row0;
  // one row's literal and separator bytes with their positions in it
  std::vector<uint32_t> tab;
  tab.reserve(unit - (uint64_t)kRtHex * ncols);
  uint32_t pos = 0;
  for (uint32_t i = 0; i <= ncols; ++i) {
    for (uint32_t b = lit_off[i]; b < lit_off[i + 1]; ++b) tab.push_back(pos++ << 8 | lit[b]);
    if (i < ncols) {
      src.hole[i] = pos;
      pos += kRtHex;
    }
  }
  for (uint32_t b = 0; b < sep_len; ++b) tab.push_back(pos++ << 8 | sep[b]);
  if (t.lazy && t.lazy->kind == Lazy::PRODUCT) {
    const Lazy& r = *t.lazy;
    src.nb = r.nb;
    for (uint32_t i = 0; i < ncols; ++i) {
      src.side[i] = r.side[i];
      src.col[i] = r.side[i] ? r.bcol(r.src[i]) : r.pcol(r.src[i]);
    }
  } else {
    // resolved, or a VIEW read in place in the index
    for (uint32_t i = 0; i < ncols; ++i) src.col[i] = t.data + (uint64_t)i * t.cap;
  }

  hipStream_t s = c.s;
  const uint32_t L = (uint32_t)tab.size();
  DBuf<uint32_t> d_tab(L, s);
  if (L) DAS_HIP(hipMemcpyAsync(d_tab.p, tab.data(), 4ull * L, hipMemcpyHostToDevice, s));
  DBuf<unsigned long long> d_bad(1, s);
  fill_dev(d_bad.p, 0, 8, s);
  DBuf<uint8_t> d_out(k, s);
  const uint64_t tiles = rt_tiles(nrows, T);
  {
    KScope ks("k_rows_text", (double)k + 20.0 * (double)nrows * ncols + 4.0 * L * (double)tiles);
    hipLaunchKernelGGL(k_rows_text, dim3(grid_for(tiles, 1, 4096)), dim3(kRtBlock), 0, s, src, (const Digest*)c.idx.digest,
                       c.idx.n_atoms, (const uint32_t*)d_tab.p, L, nrows, (uint32_t)unit, sep_len, T, k, d_out.p,
                       d_bad.p);
    DAS_HIP(hipGetLastError());
  }
  unsigned long long bad = 0;
  DAS_HIP(hipMemcpyAsync(out, d_out.p, k, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipStreamSynchronize(s));                               // the one wait: the payload
  if (n_bad) *n_bad = bad;
  return total;
}

}  // namespace das
