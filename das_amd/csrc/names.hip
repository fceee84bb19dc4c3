// Node-name search on the device (das_match_node_names, das_node_name_stats):
// the resident name heap and the DFA matcher behind
// HipDB.get_matched_node_name (redis_mongo_db.py:287-293).  DESIGN.md §3c.
//
// Heap: the nodes (cat == 1) in ascending id order, each node's name bytes
// back to back, n_nodes + 1 byte offsets.  Ids are clustered by named type
// (index.hip step 3b), so the nodes of one type are one range of that list.
// Built on the first call after an index build -- a KB that never searches
// names pays nothing -- from the context's host copy of the loader's leaf
// strings; the name of a node is its "Type name" leaf without the type name
// and the blank (AtomArrays.node_name: name_start == len(type name) + 1).
//
// Matcher: one lane per name, tiles of kNameBlock consecutive names.  The
// automaton's table and the tile's heap bytes are staged in LDS; a lane walks
// its name with one table lookup per byte and stops at the first accepting
// state (accepting states are absorbing).  The kernel knows nothing about
// regular expressions: das_name_dfa_t is the whole contract.
//
// Fetch (das_node_names): ids -> names, a gather over the same heap; its
// kernels and their comment stand below the matcher's.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "das_internal.h"

namespace das {
namespace {

constexpr unsigned kNameBlock = 256;                      // threads = names per tile
constexpr uint32_t kNameStage = DAS_NAME_STAGE_BYTES;     // a tile's names up to this many bytes are walked from LDS
// staged image: the tile's bytes from the 16-byte boundary at or below its
// first byte (head: up to 15 bytes of the previous tile), in whole uint4s
constexpr uint32_t kStageCap = kNameStage + 16;
constexpr uint32_t kStageVecs = kStageCap / 16 + 1;       // + one: the word at offset kStageCap may be read, never used
constexpr uint32_t kMaxTable = DAS_NAME_DFA_MAX_TABLE;
constexpr uint32_t kAcceptBit = 0x8000u;                  // staged table entry: next state's row base | accept << 15
static_assert(kMaxTable <= kAcceptBit, "a row base must fit below the accept bit");
static_assert(2 * kMaxTable + 256 + 16 * kStageVecs <= 64 * 1024, "table + staging within 64 KiB of LDS");

inline dim3 G(uint64_t n) { return dim3(grid_for(n, 256)); }

template <typename T>
T* dalloc(Index& idx, uint64_t count) {
  if (!count) count = 1;
  T* p = (T*)cache_alloc(sizeof(T) * count, idx.stream);
  idx.owned.push_back(p);
  idx.device_bytes += sizeof(T) * count;
  return p;
}

struct NodeFlagIn {
  const uint8_t* cat;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return cat[i] == CAT_NODE ? 1u : 0u; }
};

// node_id[pos[i]] = i for every node i (ascending ids)
__global__ void k_name_nodes(const uint8_t* cat, const uint32_t* pos, uint64_t n_atoms, uint32_t* node_id) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_atoms; i += (uint64_t)gridDim.x * blockDim.x)
    if (cat[i] == CAT_NODE) node_id[pos[i]] = (uint32_t)i;
}

// Where node j's name lies in the loader's leaf bytes.
struct NameSrc {
  const uint32_t* node_id;
  const uint32_t* name_leaf;
  const uint32_t* type;
  const uint64_t* leaf_off;
  const uint32_t* type_name_len;
  uint64_t n_leaf;
  uint32_t n_types;
  __device__ __forceinline__ uint64_t len(uint64_t j, uint64_t* begin = nullptr) const {
    const uint32_t id = node_id[j];
    const uint32_t leaf = name_leaf[id], t = type[id];
    if (leaf >= n_leaf || t >= n_types) return 0;
    const uint64_t b = leaf_off[leaf] + type_name_len[t] + 1, e = leaf_off[leaf + 1];
    if (begin) *begin = b;
    return e > b ? e - b : 0;
  }
  __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return len(j); }
};

// One thread per name: its bytes from the leaf strings to the heap; a type
// with a name byte >= 0x80 or a newline is marked (read first: most names of
// such a type would otherwise store to one line).
__global__ void k_name_gather(NameSrc src, const uint8_t* leaf_bytes, const uint64_t* off, uint64_t n, uint8_t* heap,
                              uint32_t* type_bad) {
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t b = 0;
    const uint64_t len = src.len(j, &b);
    const uint64_t o = off[j];
    uint32_t bad = 0;
    for (uint64_t k = 0; k < len; ++k) {
      const uint8_t ch = leaf_bytes[b + k];
      heap[o + k] = ch;
      bad |= (ch >= 0x80u || ch == 0x0Au) ? 1u : 0u;
    }
    const uint32_t t = src.type[src.node_id[j]];
    if (bad && t < src.n_types && !type_bad[t]) type_bad[t] = 1;
  }
}

// The range of each named type in the node list: where a run of one type
// begins and ends, and how many runs it has (one, ids being clustered).
__global__ void k_name_type_runs(const uint32_t* node_id, const uint32_t* type, uint64_t n, uint32_t n_types,
                                 uint32_t* first, uint32_t* end, uint32_t* runs) {
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t = type[node_id[j]];
    if (t >= n_types) continue;
    if (j == 0 || type[node_id[j - 1]] != t) {
      first[t] = (uint32_t)j;
      atomicAdd(&runs[t], 1u);
    }
    if (j + 1 == n || type[node_id[j + 1]] != t) end[t] = (uint32_t)(j + 1);
  }
}

__global__ void k_name_type_bytes(const uint32_t* first, const uint32_t* end, const uint32_t* runs, uint32_t n_types,
                                  const uint64_t* off, uint64_t* bytes) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_types; t += gridDim.x * blockDim.x)
    bytes[t] = runs[t] ? off[end[t]] - off[first[t]] : 0;
}

// Walks bytes [p, e) of an image readable as aligned 32-bit words
// (`word(k)` = bytes 4k .. 4k+3) from state entry `st`; returns the entry
// reached (kAcceptBit set: accepted, the walk stopped there).  The four class
// lookups of a word do not depend on the state, so only the table lookups
// form the dependent chain: one LDS latency per byte.
template <typename Word>
__device__ __forceinline__ uint32_t name_walk(Word word, uint64_t p, uint64_t e, uint32_t st, const uint16_t* s_tab,
                                              const uint8_t* s_cls) {
  if (p >= e) return st;
  for (uint64_t k = p >> 2; k <= (e - 1) >> 2; ++k) {
    const uint32_t w = word(k);
    uint32_t c[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) c[b] = s_cls[(w >> (8 * b)) & 0xFFu];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint64_t q = 4 * k + b;
      if (q >= p && q < e && !(st & kAcceptBit)) st = s_tab[st + c[b]];
    }
    if (st & kAcceptBit) break;
  }
  return st;
}

struct LdsWords {
  const uint32_t* w;
  __device__ __forceinline__ uint32_t operator()(uint64_t k) const { return w[k]; }
};
struct HeapWords {
  const uint32_t* w;
  __device__ __forceinline__ uint32_t operator()(uint64_t k) const { return w[k]; }
};

// flag[i] = 1 iff the automaton accepts the name of node lo + i, i < n.
// tab: tab_n staged entries (row base of the next state | accept bit), then
// cls: the class of each byte.  heap is 16-byte aligned and readable up to
// the 16-byte boundary above its last byte (+ 16).
__global__ void __launch_bounds__(kNameBlock) k_name_match(const uint8_t* __restrict__ heap,
                                                          const uint64_t* __restrict__ off, uint64_t lo, uint64_t n,
                                                          const uint16_t* __restrict__ tab, uint32_t tab_n,
                                                          const uint8_t* __restrict__ cls, uint32_t start,
                                                          uint32_t eot, uint8_t* __restrict__ flag) {
  __shared__ uint16_t s_tab[kMaxTable];
  __shared__ uint8_t s_cls[256];
  __shared__ uint4 s_stage[kStageVecs];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < tab_n && i < kMaxTable; i += kNameBlock) s_tab[i] = tab[i];
  s_cls[tid] = cls[tid];
  const uint64_t tiles = (n + kNameBlock - 1) / kNameBlock;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t i0 = t * kNameBlock;                                   // first name of the tile, relative to lo
    const uint64_t cnt = n - i0 < kNameBlock ? n - i0 : kNameBlock;
    const bool act = tid < cnt;
    uint64_t o0 = 0, o1 = 0;
    if (act) {
      o0 = off[lo + i0 + tid];
      o1 = off[lo + i0 + tid + 1];
    }
    const uint64_t hb = off[lo + i0], he = off[lo + i0 + cnt];            // the tile's heap bytes (block-uniform)
    const uint64_t ab = hb & ~15ull;
    const uint64_t span = he - ab;
    const uint32_t staged = span < kStageCap ? (uint32_t)span : kStageCap;
    __syncthreads();                       // the table is staged / the previous tile's walks are done
    for (uint32_t j = tid * 16; j < staged; j += kNameBlock * 16)
      s_stage[j >> 4] = *reinterpret_cast<const uint4*>(heap + ab + j);
    __syncthreads();
    if (!act) continue;
    uint32_t st = start;
    if (!(st & kAcceptBit)) {
      if (o1 - ab <= kStageCap)
        st = name_walk(LdsWords{reinterpret_cast<const uint32_t*>(s_stage)}, o0 - ab, o1 - ab, st, s_tab, s_cls);
      else                                 // reaches past the staged bytes: walked from the heap itself
        st = name_walk(HeapWords{reinterpret_cast<const uint32_t*>(heap)}, o0, o1, st, s_tab, s_cls);
      if (!(st & kAcceptBit)) st = s_tab[st + eot];
    }
    flag[i0 + tid] = (uint8_t)(st >> 15);
  }
}

struct ByteFlagIn {
  const uint8_t* f;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return f[i]; }
};

__global__ void k_name_emit(const uint8_t* flag, const uint32_t* pos, const uint32_t* node_id, uint64_t n,
                            uint32_t* out) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (flag[i]) out[pos[i]] = node_id[i];
}

void build_name_heap(Ctx& c) {
  Index& idx = c.idx;
  NameHeap& h = idx.names;
  hipStream_t s = c.s;
  const uint64_t n_atoms = idx.n_atoms, n_leaf = c.leaf_off.empty() ? 0 : c.leaf_off.size() - 1;
  const uint32_t n_types = (uint32_t)idx.n_types;
  const uint64_t before = idx.device_bytes;
  h.type_lo.assign(n_types, 0);
  h.type_hi.assign(n_types, 0);
  h.type_bytes.assign(n_types, 0);
  h.type_ascii.assign(n_types, 1);

  // nodes in ascending id order
  uint64_t nn = 0;
  if (n_atoms) {
    DBuf<uint32_t> pos(n_atoms + 1, s);
    {
      KScope ks("name_node_scan", 3.0 * n_atoms + 4.0 * n_atoms);
      nn = scan_total<uint32_t>(NodeFlagIn{idx.cat}, n_atoms, pos.p, s);
    }
    h.node_id = dalloc<uint32_t>(idx, nn);
    if (nn) {
      KScope ks("k_name_nodes", 5.0 * n_atoms + 4.0 * nn);
      hipLaunchKernelGGL(k_name_nodes, G(n_atoms), dim3(256), 0, s, (const uint8_t*)idx.cat, (const uint32_t*)pos.p,
                         n_atoms, h.node_id);
      DAS_HIP(hipGetLastError());
    }
  }
  h.n_nodes = nn;
  if (nn && n_types) {
    DAS_CHECK(n_leaf > 0 && idx.type_name_len.size() == n_types, DAS_E_INTERNAL, "name heap: no leaf strings kept");
    // name lengths -> offsets
    DBuf<uint64_t> d_loff(n_leaf + 1, s);
    DBuf<uint32_t> d_tnl(n_types, s);
    DAS_HIP(hipMemcpyAsync(d_loff.p, c.leaf_off.data(), 8 * (n_leaf + 1), hipMemcpyHostToDevice, s));
    DAS_HIP(hipMemcpyAsync(d_tnl.p, idx.type_name_len.data(), 4ull * n_types, hipMemcpyHostToDevice, s));
    const NameSrc src{h.node_id, idx.name_leaf, idx.type, d_loff.p, d_tnl.p, n_leaf, n_types};
    h.off = dalloc<uint64_t>(idx, nn + 1);
    {
      KScope ks("name_len_scan", 2.0 * 28.0 * nn + 8.0 * nn);
      h.n_bytes = scan_total<uint64_t>(src, nn, h.off, s);
    }
    // the bytes (readable in whole 16-byte loads from any 16-byte boundary inside)
    const uint64_t n_leaf_bytes = c.leaf_off[n_leaf];
    DAS_CHECK(h.n_bytes <= n_leaf_bytes && c.leaf_bytes.size() >= n_leaf_bytes, DAS_E_INTERNAL,
              "name heap: names exceed the leaf strings");
    h.bytes = dalloc<uint8_t>(idx, ((h.n_bytes + 15) & ~15ull) + 16);
    DBuf<uint8_t> d_lbytes(n_leaf_bytes ? n_leaf_bytes : 1, s);
    if (n_leaf_bytes)
      DAS_HIP(hipMemcpyAsync(d_lbytes.p, c.leaf_bytes.data(), n_leaf_bytes, hipMemcpyHostToDevice, s));
    DBuf<uint32_t> tinfo(4ull * n_types, s);                      // first, end, runs, bad
    fill_dev(tinfo.p, 0, 16ull * n_types, s);
    uint32_t *d_first = tinfo.p, *d_end = tinfo.p + n_types, *d_runs = tinfo.p + 2ull * n_types,
             *d_bad = tinfo.p + 3ull * n_types;
    {
      KScope ks("k_name_gather", 36.0 * nn + 2.0 * h.n_bytes);
      hipLaunchKernelGGL(k_name_gather, G(nn), dim3(256), 0, s, src, (const uint8_t*)d_lbytes.p,
                         (const uint64_t*)h.off, nn, h.bytes, d_bad);
      DAS_HIP(hipGetLastError());
    }
    {
      KScope ks("k_name_type_runs", 3.0 * 8.0 * nn);
      hipLaunchKernelGGL(k_name_type_runs, G(nn), dim3(256), 0, s, (const uint32_t*)h.node_id,
                         (const uint32_t*)idx.type, nn, n_types, d_first, d_end, d_runs);
      DAS_HIP(hipGetLastError());
    }
    DBuf<uint64_t> d_tbytes(n_types, s);
    {
      KScope ks("k_name_type_bytes", 36.0 * n_types);
      hipLaunchKernelGGL(k_name_type_bytes, G(n_types), dim3(256), 0, s, (const uint32_t*)d_first,
                         (const uint32_t*)d_end, (const uint32_t*)d_runs, n_types, (const uint64_t*)h.off, d_tbytes.p);
      DAS_HIP(hipGetLastError());
    }
    std::vector<uint32_t> ti(4ull * n_types);
    DAS_HIP(hipMemcpyAsync(ti.data(), tinfo.p, 16ull * n_types, hipMemcpyDeviceToHost, s));
    DAS_HIP(hipMemcpyAsync(h.type_bytes.data(), d_tbytes.p, 8ull * n_types, hipMemcpyDeviceToHost, s));
    DAS_HIP(hipStreamSynchronize(s));
    for (uint32_t t = 0; t < n_types; ++t) {
      const uint32_t runs = ti[2ull * n_types + t];
      DAS_CHECK(runs <= 1, DAS_E_UNSUPPORTED, "name heap: the nodes of a named type are not one id range");
      if (runs) {
        h.type_lo[t] = ti[t];
        h.type_hi[t] = ti[n_types + t];
        DAS_CHECK(h.type_lo[t] < h.type_hi[t] && h.type_hi[t] <= nn, DAS_E_INTERNAL, "name heap: bad type range");
      }
      h.type_ascii[t] = ti[3ull * n_types + t] ? 0 : 1;
    }
  }
  h.device_bytes = idx.device_bytes - before;
  h.built = true;
}

// ---------------------------------------------------------------------------
// Name fetch (das_node_names): ids -> names, the heap read the other way.
// Locate: one thread per input finds its id in the ascending node list (a
// binary search: no id-indexed array is kept resident for it) and notes where
// the name lies and how long it is.  A scan of the lengths gives the output
// offsets.  Copy: a tile of kNameBlock consecutive entries is one contiguous
// piece of the output; where it fits kFetchStage bytes the names are placed
// in an LDS image of that piece and the image leaves in whole 16-byte stores,
// else each name goes straight to the output.  Either way a name of up to
// kCopyWave bytes is moved by its own lane and a longer one by its wave.
// ---------------------------------------------------------------------------
constexpr uint32_t kCopyWave = DAS_NAME_COPY_WAVE;
// the image: a tile's bytes from the 16-byte boundary at or below its first; a
// tile of lane-copied names always fits
constexpr uint32_t kFetchStage = kNameBlock * kCopyWave + 16;
constexpr uint32_t kFetchVecs = kFetchStage / 16;
static_assert(kFetchStage % 16 == 0 && kFetchStage <= 64 * 1024, "the image is whole vectors within LDS");
constexpr uint32_t kMaxNameLen = 0xFFFFFFFFu;

__global__ void k_name_locate(const uint32_t* __restrict__ ids, uint64_t n, const uint8_t* __restrict__ cat,
                              uint64_t n_atoms, const uint32_t* __restrict__ node_id, uint64_t n_nodes,
                              const uint64_t* __restrict__ hoff, uint64_t n_bytes, uint64_t* __restrict__ src,
                              uint32_t* __restrict__ len, uint8_t* __restrict__ kind) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[i];
    uint64_t b = 0, l = 0;
    uint8_t k = 0;
    if (id < n_atoms && cat[id] == CAT_NODE) {
      uint64_t lo = 0, hi = n_nodes;                            // the first slot whose id is >= id
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (node_id[mid] < id) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n_nodes && node_id[lo] == id) {
        k = 1;
        const uint64_t o0 = hoff[lo], o1 = hoff[lo + 1];
        if (o0 <= o1 && o1 <= n_bytes && o1 - o0 <= kMaxNameLen) {   // a name lies inside the heap
          b = o0;
          l = o1 - o0;
        }
      }
    }
    src[i] = b;
    len[i] = (uint32_t)l;
    kind[i] = k;
  }
}

struct NameLenIn {
  const uint32_t* len;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return len[i]; }
};

// One lane: heap[s, s + len) to dst[d, d + len), the source read in aligned
// words (the word above the last byte may be read: the heap is padded).
__device__ __forceinline__ void lane_copy(uint8_t* dst, uint64_t d, const uint8_t* __restrict__ heap, uint64_t s,
                                          uint32_t len) {
  const uint32_t* hw = reinterpret_cast<const uint32_t*>(heap);
  uint32_t w = hw[s >> 2];
  for (uint32_t k = 0; k < len; ++k) {
    dst[d + k] = (uint8_t)(w >> (8 * (uint32_t)(s & 3)));
    if ((++s & 3) == 0) w = hw[s >> 2];
  }
}

// One wave (every lane calls it with the same arguments): bytes up to the
// destination's 16-byte boundary and after its last whole vector singly, the
// vectors between as 16-byte stores -- loaded as one 16-byte word where the
// source is aligned like the destination, else put together from five aligned
// 32-bit words.  `dst + d` has the alignment of d.
__device__ __forceinline__ void wave_copy(uint8_t* dst, uint64_t d, const uint8_t* __restrict__ heap, uint64_t s,
                                          uint64_t len) {
  const uint32_t lane = __lane_id();
  const uint64_t to_vec = (16 - (d & 15)) & 15;
  const uint64_t head = len < to_vec ? len : to_vec;
  if (lane < head) dst[d + lane] = heap[s + lane];
  const uint64_t nv = (len - head) >> 4;
  const uint64_t d0 = d + head, s0 = s + head;
  if ((s0 & 15) == 0) {
    for (uint64_t v = lane; v < nv; v += 64)
      *reinterpret_cast<uint4*>(dst + d0 + 16 * v) = *reinterpret_cast<const uint4*>(heap + s0 + 16 * v);
  } else {
    const uint32_t* hw = reinterpret_cast<const uint32_t*>(heap);
    const uint32_t sh = 8 * (uint32_t)(s0 & 3);
    for (uint64_t v = lane; v < nv; v += 64) {
      const uint64_t a = (s0 + 16 * v) >> 2;
      const uint32_t w0 = hw[a], w1 = hw[a + 1], w2 = hw[a + 2], w3 = hw[a + 3], w4 = hw[a + 4];
      uint4 o;
      o.x = __funnelshift_r(w0, w1, sh);
      o.y = __funnelshift_r(w1, w2, sh);
      o.z = __funnelshift_r(w2, w3, sh);
      o.w = __funnelshift_r(w3, w4, sh);
      *reinterpret_cast<uint4*>(dst + d0 + 16 * v) = o;
    }
  }
  const uint64_t done = head + 16 * nv;
  if (lane < len - done) dst[d + done + lane] = heap[s + done + lane];
}

// The names of a wave's lanes that are longer than kCopyWave, one after the
// other, each by the whole wave.  Called by every lane of the wave.
__device__ __forceinline__ void wave_copy_long(bool mine, uint8_t* dst, uint64_t d, const uint8_t* __restrict__ heap,
                                               uint64_t s, uint64_t len) {
  uint64_t m = __ballot(mine);
  while (m) {
    const int l = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const uint64_t dl = ((uint64_t)__shfl((uint32_t)(d >> 32), l, 64) << 32) | __shfl((uint32_t)d, l, 64);
    const uint64_t sl = ((uint64_t)__shfl((uint32_t)(s >> 32), l, 64) << 32) | __shfl((uint32_t)s, l, 64);
    const uint64_t ll = ((uint64_t)__shfl((uint32_t)(len >> 32), l, 64) << 32) | __shfl((uint32_t)len, l, 64);
    wave_copy(dst, dl, heap, sl, ll);
  }
}

// out[doff[i] .. doff[i + 1]) = heap[src[i] .. + len[i]) for i < n, nothing
// written at or past out[cap].  `out` is 16-byte aligned; heap as k_name_match.
__global__ void __launch_bounds__(kNameBlock) k_name_copy(const uint8_t* __restrict__ heap,
                                                         const uint64_t* __restrict__ src,
                                                         const uint32_t* __restrict__ len,
                                                         const uint64_t* __restrict__ doff, uint64_t n, uint64_t cap,
                                                         uint8_t* __restrict__ out) {
  __shared__ uint4 s_img[kFetchVecs];
  const uint32_t tid = threadIdx.x;
  const uint64_t tiles = (n + kNameBlock - 1) / kNameBlock;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t i0 = t * kNameBlock;
    const uint64_t cnt = n - i0 < kNameBlock ? n - i0 : kNameBlock;
    const uint64_t tb = doff[i0], te_all = doff[i0 + cnt];       // the tile's output bytes (block-uniform)
    const uint64_t te = te_all < cap ? te_all : cap;
    if (tb >= te) continue;                                     // nothing to write (block-uniform)
    uint64_t d = 0, s = 0;
    uint32_t l = 0;
    if (tid < cnt) {
      d = doff[i0 + tid];
      s = src[i0 + tid];
      l = len[i0 + tid];
    }
    const uint64_t ab = tb & ~15ull;
    if (te_all - ab <= kFetchStage) {
      // staged: every name of the tile into the image of out[ab, te_all)
      uint8_t* img = reinterpret_cast<uint8_t*>(s_img);
      __syncthreads();                                          // the previous tile's image was written out
      if (l && l <= kCopyWave) lane_copy(img, d - ab, heap, s, l);
      wave_copy_long(l > kCopyWave, img, d - ab, heap, s, l);
      __syncthreads();
      const uint64_t nvec = (te - ab + 15) >> 4;
      for (uint64_t v = tid; v < nvec; v += kNameBlock) {
        const uint64_t g = ab + 16 * v;
        if (g >= tb && g + 16 <= te) {
          *reinterpret_cast<uint4*>(out + g) = s_img[v];
        } else {                                                // an edge vector shared with a neighbour tile / the cap
          const uint64_t b0 = g > tb ? g : tb, b1 = g + 16 < te ? g + 16 : te;
          for (uint64_t p = b0; p < b1; ++p) out[p] = img[p - ab];
        }
      }
    } else {
      // too large for the image: each name straight to the output, cut at cap
      const uint64_t room = d < cap ? cap - d : 0;
      const uint64_t lc = l < room ? l : room;
      if (lc && l <= kCopyWave) lane_copy(out, d, heap, s, (uint32_t)lc);
      wave_copy_long(l > kCopyWave && lc, out, d, heap, s, lc);
    }
  }
}

}  // namespace

uint64_t node_names(Ctx& c, const uint32_t* h_ids, const uint32_t* d_ids, uint64_t n, uint64_t* off, uint8_t* bytes,
                    uint64_t cap, uint8_t* kind, uint64_t* n_other) {
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  DAS_CHECK(off && kind, DAS_E_INVALID, "null offset / kind buffer");
  DAS_CHECK(bytes || !cap, DAS_E_INVALID, "null name buffer");
  DAS_CHECK(h_ids || d_ids || !n, DAS_E_INVALID, "null id buffer");
  ensure_name_heap(c);
  if (n_other) *n_other = 0;
  off[0] = 0;
  if (!n) return 0;
  const NameHeap& h = c.idx.names;
  hipStream_t s = c.s;
  DBuf<uint32_t> ids_up(d_ids ? 0 : n, s);
  if (!d_ids) {
    DAS_HIP(hipMemcpyAsync(ids_up.p, h_ids, 4 * n, hipMemcpyHostToDevice, s));
    d_ids = ids_up.p;
  }
  DBuf<uint64_t> src(n, s), doff(n + 1, s);
  DBuf<uint32_t> len(n, s);
  DBuf<uint8_t> d_kind(n, s);
  {
    KScope ks("k_name_locate", 4.0 * n + 4.0 * n * (double)bits_for(h.n_nodes) + 16.0 * n + 13.0 * n);
    const uint64_t n_listed = h.node_id && h.off && h.bytes ? h.n_nodes : 0;   // (a KB without nodes has no heap)
    hipLaunchKernelGGL(k_name_locate, G(n), dim3(256), 0, s, d_ids, n, (const uint8_t*)c.idx.cat, c.idx.n_atoms,
                       (const uint32_t*)h.node_id, n_listed, (const uint64_t*)h.off, h.n_bytes, src.p, len.p,
                       d_kind.p);
    DAS_HIP(hipGetLastError());
  }
  uint64_t total = 0;
  {
    KScope ks("name_fetch_scan", 2.0 * 4.0 * n + 8.0 * n);
    total = scan_total<uint64_t>(NameLenIn{len.p}, n, doff.p, s);   // read-back 1: the total
  }
  const uint64_t k = std::min(total, cap);
  DBuf<uint8_t> d_out(k, s);
  if (k) {
    const uint64_t tiles = (n + kNameBlock - 1) / kNameBlock;
    KScope ks("k_name_copy", 2.0 * (double)k + 20.0 * n);
    hipLaunchKernelGGL(k_name_copy, dim3(grid_for(tiles, 1, 8192)), dim3(kNameBlock), 0, s, (const uint8_t*)h.bytes,
                       (const uint64_t*)src.p, (const uint32_t*)len.p, (const uint64_t*)doff.p, n, k, d_out.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(bytes, d_out.p, k, hipMemcpyDeviceToHost, s));
  }
  DAS_HIP(hipMemcpyAsync(off, doff.p, 8 * (n + 1), hipMemcpyDeviceToHost, s));
  DAS_HIP(hipMemcpyAsync(kind, d_kind.p, n, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipStreamSynchronize(s));                                  // read-back 2: the payload
  uint64_t other = 0;
  for (uint64_t i = 0; i < n; ++i) other += kind[i] ? 0 : 1;
  if (n_other) *n_other = other;
  return total;
}

void ensure_name_heap(Ctx& c) {
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  if (c.idx.names.built) return;
  const size_t owned = c.idx.owned.size();
  const uint64_t bytes = c.idx.device_bytes;
  try {
    build_name_heap(c);
  } catch (...) {
    // nothing half-built stays: the next call starts over
    (void)hipStreamSynchronize(c.s);
    while (c.idx.owned.size() > owned) {
      cache_free(c.idx.owned.back());
      c.idx.owned.pop_back();
    }
    c.idx.device_bytes = bytes;
    c.idx.names = NameHeap();
    throw;
  }
}

void check_name_dfa(const das_name_dfa_t& d) {
  DAS_CHECK(d.n_states >= 1 && d.n_states <= DAS_NAME_DFA_MAX_STATES, DAS_E_INVALID, "name DFA: n_states out of range");
  DAS_CHECK(d.n_classes >= 1 && d.n_classes <= 257, DAS_E_INVALID, "name DFA: n_classes out of range");
  DAS_CHECK((uint64_t)d.n_states * d.n_classes <= DAS_NAME_DFA_MAX_TABLE, DAS_E_INVALID,
            "name DFA: table larger than DAS_NAME_DFA_MAX_TABLE");
  DAS_CHECK(d.next && d.accept, DAS_E_INVALID, "name DFA: null table");
  DAS_CHECK(d.start < d.n_states && d.eot_class < d.n_classes, DAS_E_INVALID, "name DFA: start / eot_class out of range");
  for (int b = 0; b < 256; ++b)
    DAS_CHECK(d.byte_class[b] < d.n_classes, DAS_E_INVALID, "name DFA: byte class out of range");
  const uint32_t total = d.n_states * d.n_classes;
  for (uint32_t i = 0; i < total; ++i)
    DAS_CHECK(d.next[i] < d.n_states, DAS_E_INVALID, "name DFA: next state out of range");
  for (uint32_t s = 0; s < d.n_states; ++s) {
    DAS_CHECK(d.accept[s] <= 1, DAS_E_INVALID, "name DFA: accept is 0 or 1");
    if (!d.accept[s]) continue;
    for (uint32_t k = 0; k < d.n_classes; ++k)
      DAS_CHECK(d.accept[d.next[s * d.n_classes + k]], DAS_E_INVALID, "name DFA: an accepting state is not absorbing");
  }
}

namespace {

// The automaton as the kernels stage it: tab_n entries (the row base of the
// next state | whether it accepts), then the class of each byte.  `host` is
// the copy's source: it lives until the stream has been waited on.
struct StagedDfa {
  std::vector<uint16_t> host;
  DBuf<uint16_t> blob;
  uint32_t tab_n = 0, start = 0, eot = 0;
  const uint16_t* tab() const { return blob.p; }
  const uint8_t* cls() const { return reinterpret_cast<const uint8_t*>(blob.p + tab_n); }
};

void stage_dfa(const das_name_dfa_t& d, hipStream_t s, StagedDfa& a) {
  const uint32_t nc = d.n_classes;
  a.tab_n = d.n_states * nc;
  a.host.assign(a.tab_n + 128, 0);                                // + 256 bytes: the class of each byte
  for (uint32_t i = 0; i < a.tab_n; ++i) {
    const uint32_t t = d.next[i];
    a.host[i] = (uint16_t)(t * nc | (d.accept[t] ? kAcceptBit : 0u));
  }
  std::memcpy(a.host.data() + a.tab_n, d.byte_class, 256);
  a.start = d.start * nc | (d.accept[d.start] ? kAcceptBit : 0u);
  a.eot = d.eot_class;
  a.blob.alloc(a.host.size(), s);
  DAS_HIP(hipMemcpyAsync(a.blob.p, a.host.data(), 2 * a.host.size(), hipMemcpyHostToDevice, s));
}

// flag[i] = the automaton accepts the name of the i-th node of the type (its
// nodes are [lo, lo + n) of the node list, n > 0)
void type_flags(Ctx& c, uint32_t type_id, const StagedDfa& a, uint8_t* flag) {
  const NameHeap& h = c.idx.names;
  const uint64_t lo = h.type_lo[type_id], n = h.type_hi[type_id] - lo;
  const uint64_t tiles = (n + kNameBlock - 1) / kNameBlock;
  KScope ks("k_name_match", (double)h.type_bytes[type_id] + 8.0 * (n + 1) + (double)n);
  hipLaunchKernelGGL(k_name_match, dim3(grid_for(tiles, 1, 2048)), dim3(kNameBlock), 0, c.s, (const uint8_t*)h.bytes,
                     (const uint64_t*)h.off, lo, n, a.tab(), a.tab_n, a.cls(), a.start, a.eot, flag);
  DAS_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Names inside queries (das_table_name_filter): the rows of a binding table
// whose value in one column is a node of the type with an accepted name.  One
// lane per row finds its value's slot among the type's nodes (a binary search
// of that range of the ascending node list: a link, a node of another type,
// DAS_NONE or an id >= n_atoms is in no slot and indexes nothing) and either
// walks the name where it lies in the heap (walk) or reads the flag
// k_name_match left for that slot (flags).  Row flags -> scan -> row indices
// -> gather_table.
// ---------------------------------------------------------------------------
// The slot of `id` in node_id[type_lo, type_hi), or kNoSlot.
constexpr uint64_t kNoSlot = ~0ull;
__device__ __forceinline__ uint64_t type_slot(uint32_t id, const uint8_t* __restrict__ cat, uint64_t n_atoms,
                                              const uint32_t* __restrict__ node_id, uint64_t type_lo,
                                              uint64_t type_hi) {
  if (id >= n_atoms || cat[id] != CAT_NODE) return kNoSlot;
  uint64_t lo = type_lo, hi = type_hi;                            // the first slot of the range whose id is >= id
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (node_id[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < type_hi && node_id[lo] == id ? lo : kNoSlot;
}

// walk: flag[i] = ids[i] is a node of the type whose name the automaton
// accepts, i < n.  The table is staged as k_name_match stages it; the names
// of a tile's rows are scattered over the heap, so they are walked from it.
__global__ void __launch_bounds__(kNameBlock) k_name_filter(const uint32_t* __restrict__ ids, uint64_t n,
                                                           const uint8_t* __restrict__ cat, uint64_t n_atoms,
                                                           const uint32_t* __restrict__ node_id, uint64_t type_lo,
                                                           uint64_t type_hi, const uint64_t* __restrict__ hoff,
                                                           uint64_t n_bytes, const uint8_t* __restrict__ heap,
                                                           const uint16_t* __restrict__ tab, uint32_t tab_n,
                                                           const uint8_t* __restrict__ cls, uint32_t start,
                                                           uint32_t eot, uint8_t* __restrict__ flag) {
  __shared__ uint16_t s_tab[kMaxTable];
  __shared__ uint8_t s_cls[256];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < tab_n && i < kMaxTable; i += kNameBlock) s_tab[i] = tab[i];
  s_cls[tid] = cls[tid];
  __syncthreads();
  const uint64_t tiles = (n + kNameBlock - 1) / kNameBlock;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t i = t * kNameBlock + tid;
    if (i >= n) continue;
    uint32_t st = 0;
    const uint64_t slot = type_slot(ids[i], cat, n_atoms, node_id, type_lo, type_hi);
    if (slot != kNoSlot) {
      const uint64_t o0 = hoff[slot], o1 = hoff[slot + 1];
      if (o0 <= o1 && o1 <= n_bytes) {                            // the name lies inside the heap
        st = start;
        if (!(st & kAcceptBit)) {
          st = name_walk(HeapWords{reinterpret_cast<const uint32_t*>(heap)}, o0, o1, st, s_tab, s_cls);
          if (!(st & kAcceptBit)) st = s_tab[st + eot];
        }
      }
    }
    flag[i] = (uint8_t)(st >> 15);
  }
}

// flags: the same, from tflag[slot - type_lo] (k_name_match over the type)
__global__ void k_name_filter_flags(const uint32_t* __restrict__ ids, uint64_t n, const uint8_t* __restrict__ cat,
                                    uint64_t n_atoms, const uint32_t* __restrict__ node_id, uint64_t type_lo,
                                    uint64_t type_hi, const uint8_t* __restrict__ tflag, uint8_t* __restrict__ flag) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t slot = type_slot(ids[i], cat, n_atoms, node_id, type_lo, type_hi);
    flag[i] = slot != kNoSlot ? tflag[slot - type_lo] : (uint8_t)0;
  }
}

// idx[pos[i]] = i for every kept row i
__global__ void k_name_rows(const uint8_t* flag, const uint32_t* pos, uint64_t n, uint32_t* idx) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (flag[i]) idx[pos[i]] = (uint32_t)i;
}

void check_name_query(Ctx& c, uint32_t type_id, const das_name_dfa_t& d) {
  check_name_dfa(d);
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  DAS_CHECK(type_id < c.idx.n_types, DAS_E_INVALID, "named type id out of range");
}

}  // namespace

uint64_t match_node_names(Ctx& c, uint32_t type_id, const das_name_dfa_t& d, uint32_t* out_ids, uint64_t cap) {
  check_name_query(c, type_id, d);
  DAS_CHECK(out_ids || !cap, DAS_E_INVALID, "null id buffer");
  ensure_name_heap(c);
  const NameHeap& h = c.idx.names;
  const uint64_t lo = h.type_lo[type_id], n = h.type_hi[type_id] - lo;
  if (!n) return 0;
  hipStream_t s = c.s;
  StagedDfa a;
  stage_dfa(d, s, a);
  DBuf<uint8_t> flag(n, s);
  DBuf<uint32_t> pos(n + 1, s);
  type_flags(c, type_id, a, flag.p);
  uint64_t m = 0;
  {
    KScope ks("name_flag_scan", 2.0 * n + 4.0 * n);
    m = scan_total<uint32_t>(ByteFlagIn{flag.p}, n, pos.p, s);     // (waits: the staged table was read)
  }
  const uint64_t k = std::min(m, cap);
  if (k) {
    DBuf<uint32_t> ids(m, s);
    {
      KScope ks("k_name_emit", 5.0 * n + 8.0 * m);
      hipLaunchKernelGGL(k_name_emit, G(n), dim3(256), 0, s, (const uint8_t*)flag.p, (const uint32_t*)pos.p,
                         (const uint32_t*)h.node_id + lo, n, ids.p);
      DAS_HIP(hipGetLastError());
    }
    DAS_HIP(hipMemcpyAsync(out_ids, ids.p, 4 * k, hipMemcpyDeviceToHost, s));
    DAS_HIP(hipStreamSynchronize(s));
  }
  return m;
}

std::unique_ptr<Table> scan_node_names(Ctx& c, uint32_t type_id, const das_name_dfa_t& d, int32_t var) {
  check_name_query(c, type_id, d);
  ensure_name_heap(c);
  const NameHeap& h = c.idx.names;
  const uint64_t lo = h.type_lo[type_id], n = h.type_hi[type_id] - lo;
  if (!n) return new_table(c, DAS_TABLE_ORDERED, 1, &var, 0);
  hipStream_t s = c.s;
  StagedDfa a;
  stage_dfa(d, s, a);
  DBuf<uint8_t> flag(n, s);
  DBuf<uint32_t> pos(n + 1, s);
  type_flags(c, type_id, a, flag.p);
  uint64_t m = 0;
  {
    KScope ks("name_flag_scan", 2.0 * n + 4.0 * n);
    m = scan_total<uint32_t>(ByteFlagIn{flag.p}, n, pos.p, s);     // (waits: the staged table was read)
  }
  auto t = new_table(c, DAS_TABLE_ORDERED, 1, &var, m);
  t->nrows = m;
  if (!m) return t;
  {
    KScope ks("k_name_emit", 5.0 * n + 8.0 * m);
    hipLaunchKernelGGL(k_name_emit, G(n), dim3(256), 0, s, (const uint8_t*)flag.p, (const uint32_t*)pos.p,
                       (const uint32_t*)h.node_id + lo, n, t->col(0));
    DAS_HIP(hipGetLastError());
  }
  // the node list ascends: so does the column; its bounds are its ends
  uint32_t ends[2] = {0, kNone};
  DAS_HIP(hipMemcpyAsync(&ends[0], t->col(0), 4, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipMemcpyAsync(&ends[1], t->col(0) + (m - 1), 4, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipStreamSynchronize(s));
  t->sorted_col = 0;
  t->lo[0] = ends[0];
  t->hi[0] = ends[1];
  return t;
}

// das_table_name_filter's automatic mode: flags for a table of at least this
// many rows per node of the type, walk below.  Measured on 10^7 nodes with
// 8-byte names (profiles/name_term.json, tools/name_term_bench.py): tables of
// 10^3 .. 10^8 rows, three patterns; walk is faster up to 10^6 rows (0.27 ms
// against 0.30 ms there, 0.04 against 0.12 ms at 10^3: flags pays 0.085 ms of
// k_name_match before it looks at a row) and flags from 10^7 rows on (2.0
// against 2.3 ms, 18 against 23 ms at 10^8) -- 10^7 rows = 1 row per node, the
// smallest measured size from which flags was never slower.
constexpr uint64_t kNameFlagsRowsPerNode = 1;

// DAS_NAME_TERM_FILTER=walk|flags: the mode of every das_table_name_filter
// call that leaves it open (mode 0); otherwise by kNameFlagsRowsPerNode.
static int name_filter_mode(int mode, uint64_t rows, uint64_t type_nodes) {
  if (mode != DAS_NAME_FILTER_AUTO) return mode;
  const char* e = std::getenv("DAS_NAME_TERM_FILTER");
  if (e && !std::strcmp(e, "flags")) return DAS_NAME_FILTER_FLAGS;
  if (e && !std::strcmp(e, "walk")) return DAS_NAME_FILTER_WALK;
  return rows >= kNameFlagsRowsPerNode * type_nodes ? DAS_NAME_FILTER_FLAGS : DAS_NAME_FILTER_WALK;
}

std::unique_ptr<Table> table_name_filter(Ctx& c, const Table& t, int32_t var, uint32_t type_id,
                                         const das_name_dfa_t& d, int mode) {
  check_name_query(c, type_id, d);
  DAS_CHECK(mode >= DAS_NAME_FILTER_AUTO && mode <= DAS_NAME_FILTER_FLAGS, DAS_E_INVALID, "name filter: bad mode");
  DAS_CHECK(t.kind == DAS_TABLE_ORDERED, DAS_E_INVALID, "name filter: the table is not ordered");
  int col = -1;
  for (int k = 0; k < t.ncols && col < 0; ++k)
    if (t.vars[k] == var) col = k;
  DAS_CHECK(col >= 0, DAS_E_INVALID, "name filter: the table has no column of that variable");
  ensure_name_heap(c);
  const NameHeap& h = c.idx.names;
  const uint64_t n = t.nrows, tlo = h.type_lo[type_id], thi = h.type_hi[type_id], tn = thi - tlo;
  if (!n || !tn) return gather_table(c, t, nullptr, 0);
  DAS_CHECK(n < (1ull << 32), DAS_E_UNSUPPORTED, "name filter: too many rows");
  hipStream_t s = c.s;
  StagedDfa a;
  stage_dfa(d, s, a);
  DBuf<uint8_t> flag(n, s);
  DBuf<uint32_t> pos(n + 1, s);
  const uint32_t* ids = t.col(col);
  const double locate = 4.0 * n + 1.0 * n + 4.0 * n * (double)bits_for(tn);   // value, category, the search
  DBuf<uint8_t> tflag;
  if (name_filter_mode(mode, n, tn) == DAS_NAME_FILTER_FLAGS) {
    tflag.alloc(tn, s);
    type_flags(c, type_id, a, tflag.p);
    KScope ks("k_name_filter_flags", locate + 2.0 * n);
    hipLaunchKernelGGL(k_name_filter_flags, G(n), dim3(256), 0, s, ids, n, (const uint8_t*)c.idx.cat, c.idx.n_atoms,
                       (const uint32_t*)h.node_id, tlo, thi, (const uint8_t*)tflag.p, flag.p);
    DAS_HIP(hipGetLastError());
  } else {
    // latency-bound, as k_name_copy: a row is a chain of dependent scattered
    // loads (search, offsets, name words).  Name bytes: the type's mean.
    const uint64_t tiles = (n + kNameBlock - 1) / kNameBlock;
    KScope ks("k_name_filter", locate + 16.0 * n + (double)n * ((double)h.type_bytes[type_id] / (double)tn) + 1.0 * n);
    hipLaunchKernelGGL(k_name_filter, dim3(grid_for(tiles, 1, 2048)), dim3(kNameBlock), 0, s, ids, n,
                       (const uint8_t*)c.idx.cat, c.idx.n_atoms, (const uint32_t*)h.node_id, tlo, thi,
                       (const uint64_t*)h.off, h.n_bytes, (const uint8_t*)h.bytes, a.tab(), a.tab_n, a.cls(), a.start,
                       a.eot, flag.p);
    DAS_HIP(hipGetLastError());
  }
  uint64_t m = 0;
  {
    KScope ks("name_row_scan", 2.0 * n + 4.0 * n);
    m = scan_total<uint32_t>(ByteFlagIn{flag.p}, n, pos.p, s);     // the one read-back (waits: the staged table was read)
  }
  if (!m) return gather_table(c, t, nullptr, 0);
  DBuf<uint32_t> idx(m, s);
  {
    KScope ks("k_name_rows", 5.0 * n + 4.0 * m);
    hipLaunchKernelGGL(k_name_rows, G(n), dim3(256), 0, s, (const uint8_t*)flag.p, (const uint32_t*)pos.p, n, idx.p);
    DAS_HIP(hipGetLastError());
  }
  KScope ks("k_gather_cols", 4.0 * m + 8.0 * t.ncols * m);
  return gather_table(c, t, idx.p, m);
}

}  // namespace das
