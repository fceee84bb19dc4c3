// Atom documents of many atoms in one call (das_atoms_json, das_links_outgoing):
// what HipDB.get_atom_as_deep_representation / get_atom_as_dict answer one
// atom and one device round trip at a time (redis_mongo_db.py:187-199,
// 297-314).  DESIGN.md §3e.
//
// das_atoms_json renders json.dumps(deep representation, indent=4) as bytes:
//   expand   level 0 is the roots, level k + 1 the targets of level k's links
//            in order: a scan of the arities places them (one read-back per
//            level: the next level's size)
//   measure  deepest level first, every item the size of its piece -- its
//            indentation and its document -- as a depth-free pair (A, L):
//            the piece takes A + 4 d L bytes at indent depth d (L = its
//            lines).  A node's comes from its type text and its escaped
//            name, a link's from its children's; the separators between the
//            children (",\n", "\n" after the last) are the parent's bytes
//   place    the roots by a scan of their sizes; a link hands every child its
//            offset and its separator while it writes itself
//   write    every item its own fragments, at positions that come from the
//            scans alone (no cursor, no atomics), nothing at or past `cap`
// The text rules (escapes, UTF-8) are json_text.h's, shared with the host.
#include <algorithm>
#include <cstring>

#include "das_internal.h"
#include "json_text.h"

namespace das {
namespace {

constexpr unsigned kDocBlock = 256;
constexpr uint32_t kDocMaxDepth = DAS_DOC_MAX_DEPTH;

inline dim3 G(uint64_t n) { return dim3(grid_for(n, kDocBlock)); }

// The fragments of a document, as json.dumps(..., indent=4) writes them.
#define DOC_LIT(name, text)                  \
  __device__ const char name[] = text;       \
  constexpr uint32_t name##_n = sizeof(text) - 1
DOC_LIT(kOpen, "{\n");
DOC_LIT(kType, "\"type\": ");
DOC_LIT(kComma, ",\n");
DOC_LIT(kName, "\"name\": \"");
DOC_LIT(kNameEnd, "\"\n");
DOC_LIT(kTargets, "\"targets\": [\n");
DOC_LIT(kTargetsEnd, "]\n");
DOC_LIT(kNoTargets, "\"targets\": []\n");
DOC_LIT(kClose, "}");
DOC_LIT(kNull, "null");
#undef DOC_LIT

// Lines of a piece and the indentation they carry beyond 4 d each: a node is
// "{" "type" "name" "}" at d, d + 1, d + 1, d; a link adds the "]" line.
constexpr uint32_t kLeafLines = 4, kLeafIndent = 4 * 2;
constexpr uint32_t kLinkLines = 5, kLinkIndent = 4 * 3;
// depth-free bytes without the type text, the escaped name and the children
constexpr uint32_t kNodeA = kLeafIndent + kOpen_n + kType_n + kComma_n + kName_n + kNameEnd_n + kClose_n;
constexpr uint32_t kLink0A = kLeafIndent + kOpen_n + kType_n + kComma_n + kNoTargets_n + kClose_n;
constexpr uint32_t kLinkA = kLinkIndent + kOpen_n + kType_n + kComma_n + kTargets_n + kTargetsEnd_n + kClose_n;

struct DocIndex {
  const uint8_t* cat;
  const uint32_t* type;
  const uint32_t* ctype;
  const uint64_t* tgt_off;
  const uint32_t* tgt;
  uint64_t n_atoms;
  __device__ __forceinline__ uint8_t category(uint32_t id) const { return id < n_atoms ? cat[id] : (uint8_t)CAT_OTHER; }
  __device__ __forceinline__ bool is_link(uint32_t id) const {
    const uint8_t k = category(id);
    return k == CAT_LINK || k == CAT_LINK_REMOTE;
  }
  // targets of a link; 0 for everything else
  __device__ __forceinline__ uint64_t arity(uint32_t id, uint64_t* begin = nullptr) const {
    if (!is_link(id)) return 0;
    const uint64_t b = tgt_off[id], e = tgt_off[id + 1];
    if (begin) *begin = b;
    return e > b ? e - b : 0;
  }
};

struct ArityIn {
  DocIndex x;
  const uint32_t* ids;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return x.arity(ids[i]); }
};

// next[child0[i] ..] = the targets of item i, in stored order
__global__ void k_doc_expand(DocIndex x, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ child0,
                             uint64_t n, uint64_t n_next, uint32_t* __restrict__ next) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t b = 0;
    const uint64_t k = x.arity(ids[i], &b);
    const uint64_t c0 = child0[i];
    for (uint64_t j = 0; j < k && c0 + j < n_next; ++j) next[c0 + j] = x.tgt[b + j];
  }
}

// The resident name heap (names.hip) and the type texts of this call.
struct DocText {
  const uint32_t* node_id;
  uint64_t n_nodes;
  const uint64_t* hoff;
  uint64_t n_bytes;
  const uint8_t* heap;
  const uint8_t* type_json;
  const uint64_t* type_off;
  uint32_t n_types;
  uint64_t type_bytes;
  // where the name of node `id` lies, as k_name_locate finds it; false: not listed
  __device__ __forceinline__ bool locate(uint32_t id, uint64_t* b, uint64_t* l) const {
    uint64_t lo = 0, hi = n_nodes;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (node_id[mid] < id) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= n_nodes || node_id[lo] != id) return false;
    const uint64_t o0 = hoff[lo], o1 = hoff[lo + 1];
    *b = 0;
    *l = 0;
    if (o0 <= o1 && o1 <= n_bytes) {                         // a name lies inside the heap
      *b = o0;
      *l = o1 - o0;
    }
    return true;
  }
  // the type's JSON text ("null" for DAS_NONE); its length
  __device__ __forceinline__ uint64_t type_text(uint32_t t, const uint8_t** p) const {
    if (t < n_types) {
      const uint64_t o0 = type_off[t], o1 = type_off[t + 1];
      if (o0 <= o1 && o1 <= type_bytes) {
        *p = type_json + o0;
        return o1 - o0;
      }
    }
    *p = reinterpret_cast<const uint8_t*>(kNull);
    return kNull_n;
  }
};

struct HeapGet {
  const uint8_t* p;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return p[i]; }
};

// (A, L) of every item of one level; nA / nL: the next level's (read where the
// item is a link with targets).  ctr[0] += items that are no node and no link,
// ctr[1] += malformed name bytes.
__global__ void k_doc_measure(DocIndex x, DocText tx, const uint32_t* __restrict__ ids,
                              const uint64_t* __restrict__ child0, uint64_t n, const uint64_t* __restrict__ nA,
                              const uint64_t* __restrict__ nL, uint64_t n_next, uint64_t* __restrict__ A,
                              uint64_t* __restrict__ L, uint64_t* __restrict__ src, uint64_t* __restrict__ len,
                              unsigned long long* ctr) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[i];
    const uint8_t k = x.category(id);
    uint64_t a = 0, l = 0, b = 0, nl = 0;
    if (k == CAT_NODE && tx.locate(id, &b, &nl)) {
      const uint8_t* tp;
      uint32_t bad = 0;
      a = kNodeA + tx.type_text(x.type[id], &tp) + jt_escaped_len(HeapGet{tx.heap + b}, nl, &bad);
      l = kLeafLines;
      if (bad) atomicAdd(&ctr[1], (unsigned long long)bad);
    } else if (k == CAT_LINK || k == CAT_LINK_REMOTE) {
      const uint8_t* tp;
      const uint64_t t = tx.type_text(x.type[id], &tp);
      const uint64_t c0 = child0[i], c1 = child0[i + 1];
      if (c0 >= c1 || c1 > n_next) {
        a = kLink0A + t;
        l = kLeafLines;
      } else {
        a = kLinkA + t + 2 * (c1 - c0) - 1;                    // ",\n" between the children, "\n" after the last
        l = kLinkLines;
        for (uint64_t c = c0; c < c1; ++c) {
          a += nA[c] + 8 * nL[c];                              // the children stand two levels deeper
          l += nL[c];
        }
      }
    } else {
      atomicAdd(&ctr[0], 1ull);
    }
    A[i] = a;
    L[i] = l;
    src[i] = b;
    len[i] = nl;
  }
}

// A root's bytes at depth d0 with its separator (list dump: ",\n" / "\n").
struct RootSizeIn {
  const uint64_t* A;
  const uint64_t* L;
  uint64_t n, d0;
  uint32_t as_list;
  __device__ __forceinline__ uint64_t sep(uint64_t i) const { return as_list ? (i + 1 < n ? 2 : 1) : 0; }
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return A[i] + 4 * d0 * L[i] + sep(i); }
};

__global__ void k_doc_roots(RootSizeIn in, const uint64_t* __restrict__ roff, uint64_t base, uint64_t* __restrict__ off,
                            uint8_t* __restrict__ sep) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < in.n; i += (uint64_t)gridDim.x * blockDim.x) {
    off[i] = base + roff[i];
    sep[i] = (uint8_t)in.sep(i);
  }
}

// The output: nothing is stored at or past out[cap].
struct DocOut {
  uint8_t* out;
  uint64_t cap;
  __device__ __forceinline__ void operator()(uint64_t p, uint8_t b) const {
    if (p < cap) out[p] = b;
  }
  __device__ __forceinline__ uint64_t spaces(uint64_t p, uint64_t n) const {
    for (uint64_t k = 0; k < n; ++k) (*this)(p + k, ' ');
    return p + n;
  }
  __device__ __forceinline__ uint64_t text(uint64_t p, const void* s, uint64_t n) const {
    const uint8_t* b = static_cast<const uint8_t*>(s);
    for (uint64_t k = 0; k < n; ++k) (*this)(p + k, b[k]);
    return p + n;
  }
};

// Every item of one level (indent depth d) writes its fragments from off[i]
// and, a link, hands its children their offsets and separators.
__global__ void k_doc_write(DocIndex x, DocText tx, const uint32_t* __restrict__ ids,
                            const uint64_t* __restrict__ child0, const uint64_t* __restrict__ off,
                            const uint8_t* __restrict__ sep, const uint64_t* __restrict__ src,
                            const uint64_t* __restrict__ len, uint64_t n, uint64_t d, const uint64_t* __restrict__ nA,
                            const uint64_t* __restrict__ nL, uint64_t n_next, uint64_t* __restrict__ noff,
                            uint8_t* __restrict__ nsep, DocOut out) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[i];
    const uint8_t k = x.category(id);
    if (k != CAT_NODE && k != CAT_LINK && k != CAT_LINK_REMOTE) continue;     // counted by the measure; no text
    uint64_t p = off[i];
    const uint8_t* tp;
    const uint64_t tn = tx.type_text(x.type[id], &tp);
    p = out.spaces(p, 4 * d);
    p = out.text(p, kOpen, kOpen_n);
    p = out.spaces(p, 4 * (d + 1));
    p = out.text(p, kType, kType_n);
    p = out.text(p, tp, tn);
    p = out.text(p, kComma, kComma_n);
    p = out.spaces(p, 4 * (d + 1));
    if (k == CAT_NODE) {
      p = out.text(p, kName, kName_n);
      p = jt_escape(HeapGet{tx.heap + src[i]}, len[i], out, p);
      p = out.text(p, kNameEnd, kNameEnd_n);
    } else {
      const uint64_t c0 = child0[i], c1 = child0[i + 1];
      if (c0 >= c1 || c1 > n_next) {
        p = out.text(p, kNoTargets, kNoTargets_n);
      } else {
        p = out.text(p, kTargets, kTargets_n);
        for (uint64_t c = c0; c < c1; ++c) {
          const uint8_t s = c + 1 < c1 ? 2 : 1;
          noff[c] = p;
          nsep[c] = s;
          p += nA[c] + 4 * (d + 2) * nL[c] + s;
        }
        p = out.spaces(p, 4 * (d + 1));
        p = out.text(p, kTargetsEnd, kTargetsEnd_n);
      }
    }
    p = out.spaces(p, 4 * d);
    p = out.text(p, kClose, kClose_n);
    const uint8_t s = sep[i];
    if (s == 2) out(p++, ',');
    if (s) out(p, '\n');
  }
}

// off[n + 1] comes from the scan; the targets back to back (none at or past
// tg[cap]), and each entry's composite type and category.
__global__ void k_out_gather(DocIndex x, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ off, uint64_t n,
                             uint64_t cap, uint32_t* __restrict__ tg, uint32_t* __restrict__ ctype,
                             uint8_t* __restrict__ kind) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[i];
    const uint8_t k = x.category(id);
    uint64_t b = 0;
    const uint64_t a = x.arity(id, &b);
    const uint64_t o = off[i];
    for (uint64_t j = 0; j < a && o + j < cap; ++j) tg[o + j] = x.tgt[b + j];
    ctype[i] = (k == CAT_LINK || k == CAT_LINK_REMOTE) ? x.ctype[id] : kNone;
    kind[i] = k;
  }
}

// One level of the expansion: ids (the roots': the caller's), the first child
// of every item in the next level, and what measure and place leave per item.
struct DocLevel {
  uint64_t n = 0;
  const uint32_t* ids = nullptr;
  DBuf<uint32_t> own_ids;
  DBuf<uint64_t> child0, A, L, off, src, len;
  DBuf<uint8_t> sep;
};

DocIndex doc_index(const Index& x) {
  return DocIndex{x.cat, x.type, x.ctype, x.tgt_off, x.tgt, x.n_atoms};
}

}  // namespace

uint64_t atoms_json(Ctx& c, const uint32_t* h_ids, const uint32_t* d_ids, uint64_t n, uint32_t as_list,
                    const uint8_t* type_json, const uint64_t* type_json_off, uint32_t n_types, uint8_t* out,
                    uint64_t cap, uint64_t* n_other, uint64_t* n_bad_utf8) {
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  DAS_CHECK(as_list <= 1, DAS_E_INVALID, "as_list is 0 or 1");
  DAS_CHECK(as_list || n == 1, DAS_E_INVALID, "one root unless the text is the list dump");
  DAS_CHECK(out || !cap, DAS_E_INVALID, "null text buffer");
  DAS_CHECK(h_ids || d_ids || !n, DAS_E_INVALID, "null id buffer");
  DAS_CHECK(n_types == c.idx.n_types, DAS_E_INVALID, "one JSON text per named type of the index");
  DAS_CHECK(type_json_off && (type_json || !n_types), DAS_E_INVALID, "null type texts");
  const uint64_t type_bytes = type_json_off[n_types];
  for (uint32_t t = 0; t < n_types; ++t)
    DAS_CHECK(type_json_off[t] <= type_json_off[t + 1], DAS_E_INVALID, "type text offsets not ascending");
  ensure_name_heap(c);
  if (n_other) *n_other = 0;
  if (n_bad_utf8) *n_bad_utf8 = 0;
  if (!n) {                                                   // json.dumps([], indent=4)
    if (cap) std::memcpy(out, "[]", (size_t)std::min<uint64_t>(cap, 2));
    return 2;
  }
  const NameHeap& h = c.idx.names;
  hipStream_t s = c.s;
  const DocIndex x = doc_index(c.idx);

  DBuf<uint8_t> d_tj(type_bytes, s);
  DBuf<uint64_t> d_toff(n_types + 1ull, s);
  if (type_bytes) DAS_HIP(hipMemcpyAsync(d_tj.p, type_json, type_bytes, hipMemcpyHostToDevice, s));
  DAS_HIP(hipMemcpyAsync(d_toff.p, type_json_off, 8ull * (n_types + 1ull), hipMemcpyHostToDevice, s));
  const bool listed = h.node_id && h.off && h.bytes;           // (a KB without nodes has no heap)
  const DocText tx{h.node_id, listed ? h.n_nodes : 0, h.off, h.n_bytes, h.bytes, d_tj.p, d_toff.p, n_types, type_bytes};
  DBuf<unsigned long long> ctr(2, s);
  fill_dev(ctr.p, 0, 16, s);

  // expand
  std::vector<DocLevel> lv(1);
  lv[0].n = n;
  if (d_ids) {
    lv[0].ids = d_ids;
  } else {
    lv[0].own_ids.alloc(n, s);
    DAS_HIP(hipMemcpyAsync(lv[0].own_ids.p, h_ids, 4 * n, hipMemcpyHostToDevice, s));
    lv[0].ids = lv[0].own_ids.p;
  }
  for (;;) {
    DocLevel& cur = lv.back();
    cur.child0.alloc(cur.n + 1, s);
    uint64_t n_next = 0;
    {
      KScope ks("doc_arity_scan", 2.0 * 21.0 * cur.n + 8.0 * cur.n);
      n_next = scan_total<uint64_t>(ArityIn{x, cur.ids}, cur.n, cur.child0.p, s);   // read-back: the next level's size
    }
    if (!n_next) break;
    if (lv.size() >= kDocMaxDepth) throw Error(DAS_E_LIMIT, "atom documents nested deeper than DAS_DOC_MAX_DEPTH");
    DocLevel nx;
    nx.n = n_next;
    nx.own_ids.alloc(n_next, s);
    nx.ids = nx.own_ids.p;
    {
      KScope ks("k_doc_expand", 29.0 * cur.n + 8.0 * n_next);
      hipLaunchKernelGGL(k_doc_expand, G(cur.n), dim3(kDocBlock), 0, s, x, cur.ids, (const uint64_t*)cur.child0.p,
                         cur.n, n_next, nx.own_ids.p);
      DAS_HIP(hipGetLastError());
    }
    lv.push_back(std::move(nx));
  }

  // measure, the deepest level first
  double name_bytes = 0;
  for (size_t k = lv.size(); k-- > 0;) {
    DocLevel& cur = lv[k];
    const DocLevel* nx = k + 1 < lv.size() ? &lv[k + 1] : nullptr;
    cur.A.alloc(cur.n, s);
    cur.L.alloc(cur.n, s);
    cur.src.alloc(cur.n, s);
    cur.len.alloc(cur.n, s);
    KScope ks("k_doc_measure", 49.0 * cur.n + 4.0 * cur.n * (double)bits_for(h.n_nodes) + 16.0 * (nx ? nx->n : 0));
    hipLaunchKernelGGL(k_doc_measure, G(cur.n), dim3(kDocBlock), 0, s, x, tx, cur.ids, (const uint64_t*)cur.child0.p,
                       cur.n, nx ? (const uint64_t*)nx->A.p : nullptr, nx ? (const uint64_t*)nx->L.p : nullptr,
                       nx ? nx->n : 0, cur.A.p, cur.L.p, cur.src.p, cur.len.p, ctr.p);
    DAS_HIP(hipGetLastError());
  }

  // the roots' offsets
  const uint64_t d0 = as_list ? 1 : 0, base = as_list ? 2 : 0;         // "[\n" ... "]"
  const RootSizeIn rs{lv[0].A.p, lv[0].L.p, n, d0, as_list};
  DBuf<uint64_t> roff(n + 1, s);
  uint64_t total = 0;
  {
    KScope ks("doc_root_scan", 2.0 * 16.0 * n + 8.0 * n);
    total = base + scan_total<uint64_t>(rs, n, roff.p, s) + (as_list ? 1 : 0);   // read-back: the total
  }
  const uint64_t k = std::min(total, cap);
  DBuf<uint8_t> d_out(k, s);
  if (k) {
    lv[0].off.alloc(n, s);
    lv[0].sep.alloc(n, s);
    {
      KScope ks("k_doc_roots", 17.0 * n);
      hipLaunchKernelGGL(k_doc_roots, G(n), dim3(kDocBlock), 0, s, rs, (const uint64_t*)roff.p, base, lv[0].off.p,
                         lv[0].sep.p);
      DAS_HIP(hipGetLastError());
    }
    for (size_t l = 0; l < lv.size(); ++l) {
      DocLevel& cur = lv[l];
      DocLevel* nx = l + 1 < lv.size() ? &lv[l + 1] : nullptr;
      if (nx) {
        nx->off.alloc(nx->n, s);
        nx->sep.alloc(nx->n, s);
      }
      // the level's share of the text is not known on the host: the whole text is booked to the first level
      KScope ks("k_doc_write", 49.0 * cur.n + 25.0 * (nx ? nx->n : 0) + (l == 0 ? (double)k : 0.0));
      hipLaunchKernelGGL(k_doc_write, G(cur.n), dim3(kDocBlock), 0, s, x, tx, cur.ids, (const uint64_t*)cur.child0.p,
                         (const uint64_t*)cur.off.p, (const uint8_t*)cur.sep.p, (const uint64_t*)cur.src.p,
                         (const uint64_t*)cur.len.p, cur.n, d0 + 2 * l, nx ? (const uint64_t*)nx->A.p : nullptr,
                         nx ? (const uint64_t*)nx->L.p : nullptr, nx ? nx->n : 0, nx ? nx->off.p : nullptr,
                         nx ? nx->sep.p : nullptr, DocOut{d_out.p, k});
      DAS_HIP(hipGetLastError());
    }
    DAS_HIP(hipMemcpyAsync(out, d_out.p, k, hipMemcpyDeviceToHost, s));
  }
  unsigned long long counts[2] = {0, 0};
  DAS_HIP(hipMemcpyAsync(counts, ctr.p, 16, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipStreamSynchronize(s));                              // read-back: the text
  if (as_list) {                                                 // the list's own brackets
    if (k > 0) out[0] = '[';
    if (k > 1) out[1] = '\n';
    if (total - 1 < k) out[total - 1] = ']';
  }
  if (n_other) *n_other = counts[0];
  if (n_bad_utf8) *n_bad_utf8 = counts[1];
  return total;
}

uint64_t links_outgoing(Ctx& c, const uint32_t* h_ids, const uint32_t* d_ids, uint64_t n, uint64_t* off,
                        uint32_t* targets, uint64_t cap, uint32_t* ctype, uint8_t* kind) {
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  DAS_CHECK(off && ctype && kind, DAS_E_INVALID, "null offset / ctype / kind buffer");
  DAS_CHECK(targets || !cap, DAS_E_INVALID, "null target buffer");
  DAS_CHECK(h_ids || d_ids || !n, DAS_E_INVALID, "null id buffer");
  off[0] = 0;
  if (!n) return 0;
  hipStream_t s = c.s;
  const DocIndex x = doc_index(c.idx);
  DBuf<uint32_t> ids_up(d_ids ? 0 : n, s);
  if (!d_ids) {
    DAS_HIP(hipMemcpyAsync(ids_up.p, h_ids, 4 * n, hipMemcpyHostToDevice, s));
    d_ids = ids_up.p;
  }
  DBuf<uint64_t> d_off(n + 1, s);
  uint64_t total = 0;
  {
    KScope ks("out_arity_scan", 2.0 * 21.0 * n + 8.0 * n);
    total = scan_total<uint64_t>(ArityIn{x, d_ids}, n, d_off.p, s);          // read-back 1: the total
  }
  const uint64_t k = std::min(total, cap);
  DBuf<uint32_t> d_tg(k, s), d_ct(n, s);
  DBuf<uint8_t> d_kind(n, s);
  {
    KScope ks("k_out_gather", 38.0 * n + 8.0 * (double)k);
    hipLaunchKernelGGL(k_out_gather, G(n), dim3(kDocBlock), 0, s, x, d_ids, (const uint64_t*)d_off.p, n, k, d_tg.p,
                       d_ct.p, d_kind.p);
    DAS_HIP(hipGetLastError());
  }
  if (k) DAS_HIP(hipMemcpyAsync(targets, d_tg.p, 4 * k, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipMemcpyAsync(off, d_off.p, 8 * (n + 1), hipMemcpyDeviceToHost, s));
  DAS_HIP(hipMemcpyAsync(ctype, d_ct.p, 4 * n, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipMemcpyAsync(kind, d_kind.p, n, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipStreamSynchronize(s));                                          // read-back 2: the payload
  return total;
}

}  // namespace das
