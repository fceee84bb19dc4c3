// SimplePatternMiner's bulk steps on the device (das_halo_expand,
// das_pattern_counts, das_conjunction_counts, das_mine_combinations): the halo
// walk of notebook cell 6, the template support counts of build_patterns (cell
// 5), the counts of And-combinations of templates the mining loop asks for and
// the exhaustive search of its last cell (both at the end of this file).
// DESIGN.md §3d.
//
// Halo.  The state is four bitmaps over the atom ids (links seen / links of
// this level / atoms expanded / atoms of this level).  A level is:
//   scan    exclusive scan of the frontier's incoming degrees
//   mark    workgroups take equal tiles of incoming-list ENTRIES (not atoms: a
//           schema node sits in > 10^6 links), find each entry's atom by
//           search in the scanned degrees, filter the link on arity and the
//           pattern black list and set its bit (lanes of a wave that hit one
//           word merge first; a bit already set is not set again)
//   compact new = level & ~seen -> ascending ids; seen |= level; level = 0
//           (count per block, then emit; 16-byte loads and stores)
//   targets each new link's targets set their bits in the atom bitmap
//   compact the new atoms = the next frontier, with the sum of their degrees
// and one read-back of three counts (links, atoms, next entries).
//
// Counts.  Templates are generated per (link, mask), sorted and merged; one
// thread per distinct template resolves its key (type << 32 | target) in
// P_{a,p} -- one grounded target: the key range's width; two, where the rows
// of a key are sorted by the other: an equal range inside it.  Targets (1,2)
// of arity 3 are a prefix of neither index: the shorter of the two key ranges
// is scanned for the other target, in chunks of DAS_PC_CHUNK_ROWS rows, one
// wave per chunk and one add per wave (a short range is one chunk, a hub's
// range is spread over the grid).
#include <algorithm>
#include <cstring>

#include "das_internal.h"
#include "md5.h"
#include "mx_unrank.h"

namespace das {
namespace {

constexpr unsigned kB = 256;
constexpr uint32_t kHaloTile = DAS_HALO_BLOCK_ENTRIES;    // entries of one workgroup pass
constexpr uint32_t kPcChunk = DAS_PC_CHUNK_ROWS;          // rows of one wave step
constexpr uint32_t kBitBlocks = 1024;                     // workgroups of a bitmap compaction (at most)
constexpr uint32_t kInvalidKey = 1u << 26;                // sort key of a dropped template (after every arity << 24 | type)
static_assert(kHaloTile % kB == 0 && kPcChunk % 64 == 0, "tiles are whole waves");

inline dim3 G(uint64_t n, unsigned cap = 65535u * 8u) { return dim3(grid_for(n, kB, cap)); }

// ---------------------------------------------------------------------------
// halo
// ---------------------------------------------------------------------------
struct DegIn {
  const uint32_t* frontier;
  const uint32_t* in_off;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
    const uint32_t a = frontier[i];
    return (uint64_t)(in_off[a + 1] - in_off[a]);
  }
  static std::string name() { return "DegIn"; }
};

// bits of the seeds in the level's atom bitmap (ids checked on the host)
__global__ void k_halo_seed_bits(const uint32_t* seeds, uint64_t n, uint32_t* level_atoms, unsigned long long* deg_sum) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *deg_sum = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = seeds[i];
    atomicOr(&level_atoms[a >> 5], 1u << (a & 31));
  }
}

// eoff: exclusive scan of the frontier's incoming degrees, E their sum.
// Entry e belongs to the last frontier atom a with eoff[a] <= e.
__global__ void __launch_bounds__(kB) k_halo_mark_links(const uint32_t* __restrict__ frontier, uint64_t nf,
                                                       const uint64_t* __restrict__ eoff, uint64_t E,
                                                       const uint32_t* __restrict__ in_off,
                                                       const uint32_t* __restrict__ in_link,
                                                       const uint32_t* __restrict__ arity,
                                                       const uint32_t* __restrict__ type,
                                                       const uint8_t* __restrict__ blocked, uint32_t n_types,
                                                       uint64_t n_atoms, uint32_t* level_links) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t tiles = (E + kHaloTile - 1) / kHaloTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t wbase = t * kHaloTile + (uint64_t)wave * (kHaloTile / (kB / 64));
    for (uint32_t it = 0; it < kHaloTile / kB; ++it) {
      const uint64_t e = wbase + it * 64 + lane;
      uint32_t word = kNone, bits = 0;
      if (e < E) {
        uint64_t lo = 0, hi = nf;
        while (lo < hi) {
          const uint64_t mid = (lo + hi) >> 1;
          if (eoff[mid] <= e) lo = mid + 1; else hi = mid;
        }
        const uint64_t a = lo - 1;                       // eoff[0] = 0 <= e: lo >= 1
        const uint32_t atom = frontier[a];
        const uint32_t link = in_link[(uint64_t)in_off[atom] + (e - eoff[a])];
        if (link < n_atoms) {
          const uint32_t ar = arity[link], ty = type[link];
          if ((ar == 2 || ar == 3) && ty < n_types && !(blocked && blocked[ty])) {
            word = link >> 5;
            bits = 1u << (link & 31);
            if (level_links[word] & bits) {              // set already (a stale read only repeats the atomic)
              word = kNone;
              bits = 0;
            }
          }
        }
      }
      // an atom's list is sorted by link id: the lanes of one word are
      // neighbours, and the first of them sets the bits of all
      const uint32_t prev = __shfl_up(word, 1, 64);
      uint32_t acc = bits;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ow = __shfl_down(word, d, 64), ob = __shfl_down(acc, d, 64);
        if (lane + d < 64 && ow == word) acc |= ob;
      }
      if (bits && (lane == 0 || prev != word)) atomicOr(&level_links[word], acc);
    }
  }
}

// every target of the n = *n_links new links that was in no frontier yet
__global__ void k_halo_mark_targets(const uint32_t* __restrict__ links, const unsigned long long* n_links,
                                    const uint64_t* __restrict__ tgt_off, const uint32_t* __restrict__ tgt,
                                    uint64_t n_atoms, const uint32_t* __restrict__ seen_atoms, uint32_t* level_atoms,
                                    unsigned long long* deg_sum) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *deg_sum = 0;     // the compaction after this kernel adds to it
  const uint64_t n = *n_links;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t l = links[i];
    const uint64_t b = tgt_off[l];
    const uint32_t k = (uint32_t)min((uint64_t)3, tgt_off[l + 1] - b);   // arity 2 or 3 (mark_links)
    for (uint32_t p = 0; p < k; ++p) {
      const uint32_t t = tgt[b + p];
      if (t >= n_atoms) continue;
      const uint32_t w = t >> 5, bit = 1u << (t & 31);
      if ((seen_atoms[w] & bit) || (level_atoms[w] & bit)) continue;     // (a stale read only repeats the atomic)
      atomicOr(&level_atoms[w], bit);
    }
  }
}

__device__ __forceinline__ uint32_t popc_new(const uint4& L, const uint4& S) {
  return __popc(L.x & ~S.x) + __popc(L.y & ~S.y) + __popc(L.z & ~S.z) + __popc(L.w & ~S.w);
}

// counts[b] = bits of level & ~seen in block b's vectors [b * per, (b + 1) * per)
__global__ void __launch_bounds__(kB) k_bits_count(const uint4* __restrict__ level, const uint4* __restrict__ seen,
                                                  uint64_t nvec, uint64_t per, uint32_t* counts) {
  __shared__ uint32_t s_w[kB / 64];
  const uint64_t v0 = blockIdx.x * per, v1 = min(v0 + per, nvec);
  uint32_t local = 0;
  for (uint64_t v = v0 + threadIdx.x; v < v1; v += kB) {
    const uint4 L = level[v];
    if (L.x | L.y | L.z | L.w) local += popc_new(L, seen[v]);
  }
  local = wave_reduce_sum(local);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (unsigned w = 0; w < kB / 64; ++w) t += s_w[w];
    counts[blockIdx.x] = t;
  }
}

// out: the ids of level & ~seen, ascending; seen |= level; level = 0; *total
// = their number; with in_off, *deg_sum += the incoming degrees of the ids.
__global__ void __launch_bounds__(kB) k_bits_emit(uint4* level, uint4* seen, uint64_t nvec, uint64_t per,
                                                 const uint32_t* __restrict__ counts, uint32_t* out,
                                                 unsigned long long* total, const uint32_t* __restrict__ in_off,
                                                 unsigned long long* deg_sum) {
  __shared__ uint32_t s_w[kB / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t pre = 0;
  for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kB) pre += counts[i];
  pre = wave_reduce_sum(pre);
  if (lane == 0) s_w[wave] = pre;
  __syncthreads();
  uint32_t run = 0;
  for (unsigned w = 0; w < kB / 64; ++w) run += s_w[w];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = (unsigned long long)run + counts[blockIdx.x];
  __syncthreads();
  const uint64_t v0 = blockIdx.x * per, v1 = min(v0 + per, nvec);
  unsigned long long deg = 0;
  for (uint64_t tb = v0; tb < v1; tb += kB) {
    const uint64_t v = tb + threadIdx.x;
    uint32_t nw[4] = {0, 0, 0, 0};
    if (v < v1) {
      const uint4 L = level[v];
      if (L.x | L.y | L.z | L.w) {
        const uint4 S = seen[v];
        nw[0] = L.x & ~S.x; nw[1] = L.y & ~S.y; nw[2] = L.z & ~S.z; nw[3] = L.w & ~S.w;
        seen[v] = make_uint4(S.x | L.x, S.y | L.y, S.z | L.z, S.w | L.w);
        level[v] = make_uint4(0, 0, 0, 0);
      }
    }
    const uint32_t cnt = __popc(nw[0]) + __popc(nw[1]) + __popc(nw[2]) + __popc(nw[3]);
    const uint32_t inc = wave_incl_sum_u32(cnt);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t wpre = 0, all = 0;
    for (unsigned w = 0; w < kB / 64; ++w) {
      wpre += w < wave ? s_w[w] : 0u;
      all += s_w[w];
    }
    if (cnt) {
      uint32_t pos = run + wpre + inc - cnt;
      const uint32_t base = (uint32_t)(v * 128);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t bits = nw[w];
        while (bits) {
          const uint32_t id = base + 32 * w + (uint32_t)(__ffs(bits) - 1);
          bits &= bits - 1;
          out[pos++] = id;
          if (in_off) deg += in_off[id + 1] - in_off[id];
        }
      }
    }
    run += all;
    __syncthreads();
  }
  if (in_off) {
    deg = wave_reduce_sum(deg);
    if (lane == 0 && deg) atomicAdd(deg_sum, deg);
  }
}

struct HaloState {
  uint64_t nvec = 0, per = 0;
  unsigned blocks = 1;
  DBuf<uint32_t> bits;            // links seen | links level | atoms seen | atoms level
  DBuf<uint32_t> counts;          // per-block counts of a compaction
  DBuf<unsigned long long> ctr;   // new links, new atoms, next entries
  uint4* vec(int k) const { return reinterpret_cast<uint4*>(bits.p) + k * nvec; }
  uint32_t* words(int k) const { return bits.p + 4 * k * nvec; }
};

// new = level & ~seen of bitmap pair (k_seen, k_seen + 1) -> out, ascending
void compact_bits(Ctx& c, HaloState& h, int k_seen, uint32_t* out, unsigned long long* total, const uint32_t* in_off) {
  {
    ProfScope ps(c, "k_bits_count", 32.0 * h.nvec);
    hipLaunchKernelGGL(k_bits_count, dim3(h.blocks), dim3(kB), 0, c.s, (const uint4*)h.vec(k_seen + 1),
                       (const uint4*)h.vec(k_seen), h.nvec, h.per, h.counts.p);
    DAS_HIP(hipGetLastError());
  }
  ProfScope ps(c, "k_bits_emit", 32.0 * h.nvec);
  hipLaunchKernelGGL(k_bits_emit, dim3(h.blocks), dim3(kB), 0, c.s, h.vec(k_seen + 1), h.vec(k_seen), h.nvec, h.per,
                     (const uint32_t*)h.counts.p, out, total, in_off, h.ctr.p + 2);
  DAS_HIP(hipGetLastError());
}

void read_counters3(Ctx& c, const HaloState& h, uint64_t out[3]) {
  DAS_HIP(hipMemcpyAsync(c.scratch.h, h.ctr.p, 24, hipMemcpyDeviceToHost, c.s));
  DAS_HIP(hipStreamSynchronize(c.s));
  count_readback();
  for (int i = 0; i < 3; ++i) out[i] = c.scratch.h[i];
}

std::unique_ptr<Table> id_column(Ctx& c, const uint32_t* d_ids, uint64_t n, uint64_t n_atoms) {
  const int32_t var0 = 0;
  auto t = new_table(c, DAS_TABLE_ORDERED, 1, &var0, n);
  t->nrows = n;
  t->sorted_col = 0;
  if (n_atoms) t->hi[0] = (uint32_t)(n_atoms - 1);
  if (n) copy_dev(t->col(0), d_ids, 4 * n, c.s);
  return t;
}

void miner_check(const Ctx& c) {
  DAS_CHECK(c.idx.built, DAS_E_NOT_BUILT, "index not built");
  DAS_CHECK(c.idx.shard_world <= 1, DAS_E_UNSUPPORTED, "pattern miner: a sharded index holds only its own links' rows");
}

// device copy of the black-list flags per named type (null: no list)
void upload_blocked(Ctx& c, DBuf<uint8_t>& d) {
  const Index& idx = c.idx;
  if (!idx.no_pattern_any || idx.no_pattern.empty()) return;
  d.alloc(idx.no_pattern.size(), c.s);
  DAS_HIP(hipMemcpyAsync(d.p, idx.no_pattern.data(), idx.no_pattern.size(), hipMemcpyHostToDevice, c.s));
}

}  // namespace

void halo_expand(Ctx& c, const uint32_t* seed_ids, uint64_t n_seeds, uint32_t levels,
                 std::vector<std::unique_ptr<Table>>& links, std::vector<std::unique_ptr<Table>>& atoms) {
  miner_check(c);
  Index& idx = c.idx;
  DAS_CHECK(levels <= DAS_HALO_MAX_LEVELS, DAS_E_INVALID, "halo: more than DAS_HALO_MAX_LEVELS levels");
  DAS_CHECK(seed_ids || !n_seeds, DAS_E_INVALID, "halo: null seed ids");
  DAS_CHECK(n_seeds < (1ull << 32), DAS_E_INVALID, "halo: too many seeds");
  for (uint64_t i = 0; i < n_seeds; ++i)
    DAS_CHECK(seed_ids[i] < idx.n_atoms, DAS_E_INVALID, "halo: seed id out of range");
  links.clear();
  atoms.clear();
  hipStream_t s = c.s;
  const uint64_t n_atoms = idx.n_atoms;
  uint64_t nf = 0, E = 0;
  HaloState h;
  DBuf<uint32_t> d_seeds, scratch_l, scratch_a, frontier0;
  DBuf<uint8_t> blocked;
  DBuf<uint64_t> eoff;
  const uint32_t* frontier = nullptr;
  if (levels && n_seeds) {
    h.nvec = (n_atoms + 127) / 128;
    h.blocks = grid_for(h.nvec, kB, kBitBlocks);
    h.per = (h.nvec + h.blocks - 1) / h.blocks;
    h.bits.alloc(16 * h.nvec, s);
    h.counts.alloc(h.blocks, s);
    h.ctr.alloc(4, s);
    fill_dev(h.bits.p, 0, 64 * h.nvec, s);
    fill_dev(h.ctr.p, 0, 32, s);
    upload_blocked(c, blocked);
    scratch_l.alloc(std::max<uint64_t>(idx.n_links, 1), s);
    scratch_a.alloc(n_atoms, s);
    d_seeds.alloc(n_seeds, s);
    DAS_HIP(hipMemcpyAsync(d_seeds.p, seed_ids, 4 * n_seeds, hipMemcpyHostToDevice, s));
    {
      ProfScope ps(c, "k_halo_seed_bits", 8.0 * n_seeds);
      hipLaunchKernelGGL(k_halo_seed_bits, G(n_seeds, 1024), dim3(kB), 0, s, (const uint32_t*)d_seeds.p, n_seeds,
                         h.words(3), h.ctr.p + 2);
      DAS_HIP(hipGetLastError());
    }
    compact_bits(c, h, 2, scratch_a.p, h.ctr.p + 1, idx.in_off);
    uint64_t r[3];
    read_counters3(c, h, r);
    nf = r[1];
    E = r[2];
    frontier0.alloc(std::max<uint64_t>(nf, 1), s);
    if (nf) copy_dev(frontier0.p, scratch_a.p, 4 * nf, s);
    frontier = frontier0.p;
  }
  for (uint32_t lv = 0; lv < levels; ++lv) {
    uint64_t nl = 0, na = 0, e_next = 0;
    if (nf && E) {
      DAS_CHECK(E <= idx.in_total, DAS_E_INTERNAL, "halo: more entries than incoming links");
      if (eoff.n < nf) eoff.alloc(nf, s);
      exclusive_scan_fn<uint64_t>(DegIn{frontier, idx.in_off}, nf, eoff.p, s);
      {
        ProfScope ps(c, "k_halo_mark_links", 12.0 * E + 16.0 * nf);
        hipLaunchKernelGGL(k_halo_mark_links, dim3(grid_for(E, kHaloTile, 4096)), dim3(kB), 0, s, frontier, nf,
                           (const uint64_t*)eoff.p, E, (const uint32_t*)idx.in_off, (const uint32_t*)idx.in_link,
                           (const uint32_t*)idx.arity, (const uint32_t*)idx.type, (const uint8_t*)blocked.p,
                           (uint32_t)idx.n_types, n_atoms, h.words(1));
        DAS_HIP(hipGetLastError());
      }
      compact_bits(c, h, 0, scratch_l.p, h.ctr.p + 0, nullptr);
      const uint64_t bound = std::min<uint64_t>(E, idx.n_links);       // new links at most
      {
        ProfScope ps(c, "k_halo_mark_targets", 32.0 * bound);
        hipLaunchKernelGGL(k_halo_mark_targets, G(bound, 4096), dim3(kB), 0, s, (const uint32_t*)scratch_l.p,
                           (const unsigned long long*)h.ctr.p, (const uint64_t*)idx.tgt_off,
                           (const uint32_t*)idx.tgt, n_atoms, (const uint32_t*)h.words(2), h.words(3), h.ctr.p + 2);
        DAS_HIP(hipGetLastError());
      }
      compact_bits(c, h, 2, scratch_a.p, h.ctr.p + 1, idx.in_off);
      uint64_t r[3];
      read_counters3(c, h, r);
      nl = r[0];
      na = r[1];
      e_next = r[2];
      DAS_CHECK(nl <= idx.n_links && na <= n_atoms, DAS_E_INTERNAL, "halo: level larger than the index");
    }
    links.push_back(id_column(c, scratch_l.p, nl, n_atoms));
    atoms.push_back(id_column(c, scratch_a.p, na, n_atoms));
    frontier = atoms.back()->col(0);
    nf = na;
    E = e_next;
  }
}

// ---------------------------------------------------------------------------
// template support
// ---------------------------------------------------------------------------
namespace {

struct PView {
  const uint64_t* ukey;
  const uint64_t* uoff;
  uint64_t nkeys;
  const uint32_t* col[3];      // t0 .. t2 of the rows
};
struct PcIndex {
  PView p2[2], p3[3];
};
PView view_of(const PosIndex& P, int arity) {
  PView v{};
  v.ukey = P.ukey;
  v.uoff = P.uoff;
  v.nkeys = P.ukey && P.uoff ? P.nkeys : 0;
  for (int k = 0; k < arity; ++k) v.col[k] = P.t.data ? P.t.col(1 + k) : nullptr;
  return v;
}

// rows [lo, hi) of key (ty, t); false: no such key
__device__ __forceinline__ bool key_run(const PView& P, uint32_t ty, uint32_t t, uint64_t& lo, uint64_t& hi) {
  const uint64_t key = ((uint64_t)ty << 32) | t;
  uint64_t a = 0, b = P.nkeys;
  while (a < b) {
    const uint64_t mid = (a + b) >> 1;
    if (P.ukey[mid] < key) a = mid + 1; else b = mid;
  }
  lo = hi = 0;
  if (a >= P.nkeys || P.ukey[a] != key) return false;
  lo = P.uoff[a];
  hi = P.uoff[a + 1];
  return true;
}
// first row of [lo, hi) whose col value is >= v (col ascending there)
__device__ __forceinline__ uint64_t lower_row(const uint32_t* col, uint64_t lo, uint64_t hi, uint64_t v) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)col[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Row i * 6 + j: template j of link i (build_patterns: arity 2 -> 2, arity 3
// -> 6; bit p of the mask = target p grounded).  k0 = arity << 24 | type, or
// kInvalidKey: no such template, or a grounded target that is not a node.
// A wildcard or unused position holds n_atoms (sorts after every id).
__global__ void k_pc_templates(const uint32_t* __restrict__ links, uint64_t n, uint64_t n_atoms, uint32_t n_types,
                               const uint8_t* __restrict__ cat, const uint32_t* __restrict__ arity,
                               const uint32_t* __restrict__ type, const uint64_t* __restrict__ tgt_off,
                               const uint32_t* __restrict__ tgt, uint32_t* k0, uint32_t* t0, uint32_t* t1,
                               uint32_t* t2) {
  const uint64_t R = n * 6;
  const uint32_t W = (uint32_t)n_atoms;
  for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < R; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = r / 6;
    const uint32_t j = (uint32_t)(r % 6);
    const uint32_t l = links[i];
    uint32_t key = kInvalidKey, T[3] = {W, W, W};
    if (l < n_atoms && cat[l] == CAT_LINK) {
      const uint32_t ar = arity[l], ty = type[l];
      const uint64_t o = tgt_off[l];
      uint32_t mask = 0;
      if (ar == 2 && j < 2) mask = j == 0 ? 2u : 1u;
      else if (ar == 3) mask = j == 0 ? 6u : j == 1 ? 5u : j == 2 ? 3u : j == 3 ? 4u : j == 4 ? 2u : 1u;
      if (mask && ty < n_types && tgt_off[l + 1] - o == ar) {
        bool ok = true;
        for (uint32_t p = 0; p < ar; ++p) {
          if (!((mask >> p) & 1u)) continue;
          const uint32_t t = tgt[o + p];
          if (t >= n_atoms || cat[t] != CAT_NODE) ok = false;   // get_node_type raises: the template is dropped
          T[p] = t;
        }
        if (ok) key = (ar << 24) | ty;
        else T[0] = T[1] = T[2] = W;
      }
    }
    k0[r] = key;
    t0[r] = T[0];
    t1[r] = T[1];
    t2[r] = T[2];
  }
}

// flag[i] = 1: sorted row i is a template and differs from the row before it
__global__ void k_pc_flags(const uint32_t* __restrict__ k0, const uint32_t* __restrict__ t0,
                           const uint32_t* __restrict__ t1, const uint32_t* __restrict__ t2,
                           const uint32_t* __restrict__ perm, uint64_t R, uint32_t* flag) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < R; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = perm[i];
    uint32_t f = k0[r] != kInvalidKey ? 1u : 0u;
    if (f && i > 0) {
      const uint32_t q = perm[i - 1];
      if (k0[q] == k0[r] && t0[q] == t0[r] && t1[q] == t1[r] && t2[q] == t2[r]) f = 0;
    }
    flag[i] = f;
  }
}

__global__ void k_pc_emit(const uint32_t* __restrict__ k0, const uint32_t* __restrict__ t0,
                          const uint32_t* __restrict__ t1, const uint32_t* __restrict__ t2,
                          const uint32_t* __restrict__ perm, const uint32_t* __restrict__ flag,
                          const uint32_t* __restrict__ pos, uint64_t R, uint32_t* o_ar, uint32_t* o_ty, uint32_t* o_t0,
                          uint32_t* o_t1, uint32_t* o_t2) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < R; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!flag[i]) continue;
    const uint32_t r = perm[i], o = pos[i];
    o_ar[o] = k0[r] >> 24;
    o_ty[o] = k0[r] & 0xFFFFFFu;
    o_t0[o] = t0[r];
    o_t1[o] = t1[r];
    o_t2[o] = t2[r];
  }
}

__device__ __forceinline__ bool digest_less(const Digest& a, const Digest& b) {
  return a.hi() != b.hi() ? a.hi() < b.hi() : a.lo() < b.lo();
}

// One thread per template: its count where a key range answers it; else the
// range to scan: rows [p_lo, p_lo + p_len) of P_{3,p_sel}, counting those
// whose other grounded target equals p_val, in nch chunks.
__global__ void k_pc_resolve(uint64_t m, uint32_t W, const uint32_t* __restrict__ c_ar,
                             const uint32_t* __restrict__ c_ty, const uint32_t* __restrict__ c_t0,
                             const uint32_t* __restrict__ c_t1, const uint32_t* __restrict__ c_t2, PcIndex X,
                             const uint8_t* __restrict__ blocked, uint32_t unord0, uint32_t unord1,
                             const Digest* __restrict__ digest, unsigned long long* count, uint64_t* nch,
                             uint64_t* p_lo, uint64_t* p_len, uint32_t* p_sel, uint32_t* p_val) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ar = c_ar[i], ty = c_ty[i];
    uint32_t T[3] = {c_t0[i], c_t1[i], c_t2[i]};
    unsigned long long cnt = 0;
    uint64_t chunks = 0, lo = 0, hi = 0;
    uint32_t sel = 0, val = 0;
    if (!(blocked && blocked[ty]) && (ar == 2 || ar == 3)) {
      uint32_t g[3], ng = 0;
      for (uint32_t p = 0; p < ar; ++p)
        if (T[p] != W) g[ng++] = T[p];
      if (ty == unord0 || ty == unord1) {
        // the reference's key: sorted(handles), '*' before every hex digit
        if (ng == 2 && digest_less(digest[g[1]], digest[g[0]])) {
          const uint32_t x = g[0];
          g[0] = g[1];
          g[1] = x;
        }
        for (uint32_t p = 0; p < ar; ++p) T[p] = p + ng < ar ? W : g[p + ng - ar];
      }
      if (ng == 1) {
        uint32_t p = 0;
        while (T[p] == W) ++p;
        if (key_run(ar == 2 ? X.p2[p] : X.p3[p], ty, T[p], lo, hi)) cnt = hi - lo;
      } else if (ng == 2 && ar == 3) {
        if (T[2] == W) {                       // (0,1): rows of key t0 are sorted by t1
          if (key_run(X.p3[0], ty, T[0], lo, hi))
            cnt = lower_row(X.p3[0].col[1], lo, hi, (uint64_t)T[1] + 1) - lower_row(X.p3[0].col[1], lo, hi, T[1]);
        } else if (T[1] == W) {                // (0,2): rows of key t2 are sorted by t0
          if (key_run(X.p3[2], ty, T[2], lo, hi))
            cnt = lower_row(X.p3[2].col[0], lo, hi, (uint64_t)T[0] + 1) - lower_row(X.p3[2].col[0], lo, hi, T[0]);
        } else {                               // (1,2): the shorter key range, filtered on the other target
          uint64_t lo1, hi1, lo2, hi2;
          if (key_run(X.p3[1], ty, T[1], lo1, hi1) && key_run(X.p3[2], ty, T[2], lo2, hi2)) {
            if (hi1 - lo1 <= hi2 - lo2) { sel = 1; val = T[2]; lo = lo1; hi = hi1; }
            else { sel = 2; val = T[1]; lo = lo2; hi = hi2; }
            chunks = (hi - lo + kPcChunk - 1) / kPcChunk;
          }
        }
      }
    }
    count[i] = cnt;
    nch[i] = chunks;
    p_lo[i] = lo;
    p_len[i] = chunks ? hi - lo : 0;
    p_sel[i] = sel;
    p_val[i] = val;
  }
}

// choff: exclusive scan of nch.  One wave per chunk.
__global__ void __launch_bounds__(kB) k_pc_scan(uint64_t m, const uint64_t* __restrict__ choff,
                                               const uint64_t* __restrict__ nch, const uint64_t* __restrict__ p_lo,
                                               const uint64_t* __restrict__ p_len, const uint32_t* __restrict__ p_sel,
                                               const uint32_t* __restrict__ p_val, const uint32_t* __restrict__ col31_t2,
                                               const uint32_t* __restrict__ col32_t1, unsigned long long* count) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total = choff[m - 1] + nch[m - 1];
  const uint64_t nwaves = (uint64_t)gridDim.x * (kB / 64);
  for (uint64_t ch = (uint64_t)blockIdx.x * (kB / 64) + (threadIdx.x >> 6); ch < total; ch += nwaves) {
    uint64_t a = 0, b = m;                     // the last template with choff <= ch owns the chunk
    while (a < b) {
      const uint64_t mid = (a + b) >> 1;
      if (choff[mid] <= ch) a = mid + 1; else b = mid;
    }
    const uint64_t i = a - 1;
    const uint64_t r0 = p_lo[i] + (ch - choff[i]) * kPcChunk;
    const uint64_t r1 = min(r0 + kPcChunk, p_lo[i] + p_len[i]);
    const uint32_t* col = p_sel[i] == 1 ? col31_t2 : col32_t1;
    const uint32_t val = p_val[i];
    uint32_t cnt = 0;
    for (uint64_t r = r0 + lane; r < r1; r += 64) cnt += col[r] == val ? 1u : 0u;
    cnt = wave_reduce_sum(cnt);
    if (lane == 0 && cnt) atomicAdd(&count[i], (unsigned long long)cnt);
  }
}

__global__ void k_pc_finish(uint64_t m, uint32_t W, const unsigned long long* __restrict__ count, uint32_t* t0,
                            uint32_t* t1, uint32_t* t2, uint32_t* c_lo, uint32_t* c_hi) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    if (t0[i] == W) t0[i] = kNone;
    if (t1[i] == W) t1[i] = kNone;
    if (t2[i] == W) t2[i] = kNone;
    c_lo[i] = (uint32_t)count[i];
    c_hi[i] = (uint32_t)(count[i] >> 32);
  }
}

uint32_t type_named(const Index& idx, const char* name) {
  Digest d;
  md5::digest_bytes(reinterpret_cast<const uint8_t*>(name), std::strlen(name), d.w);
  for (uint32_t t = 0; t < idx.type_digest.size(); ++t)
    if (std::memcmp(d.w, idx.type_digest[t].w, 16) == 0) return t;
  return kNone;
}

}  // namespace

std::unique_ptr<Table> pattern_counts(Ctx& c, const uint32_t* d_links, uint64_t n) {
  miner_check(c);
  Index& idx = c.idx;
  DAS_CHECK(n < (1ull << 32) / 6, DAS_E_UNSUPPORTED, "pattern counts: too many links in one call");
  hipStream_t s = c.s;
  const int32_t vars[7] = {0, 1, 2, 3, 4, 5, 6};
  const uint64_t n_atoms = idx.n_atoms, R = 6 * n;
  const uint32_t W = (uint32_t)n_atoms;
  uint64_t m = 0;
  DBuf<uint32_t> rows, perm, flag, pos;
  if (R) {
    rows.alloc(4 * R, s);
    uint32_t *k0 = rows.p, *t0 = rows.p + R, *t1 = rows.p + 2 * R, *t2 = rows.p + 3 * R;
    {
      ProfScope ps(c, "k_pc_templates", 4.0 * n + 6.0 * n * 16.0 + n * (9.0 + 8.0 + 12.0 + 3.0));
      hipLaunchKernelGGL(k_pc_templates, G(R), dim3(kB), 0, s, d_links, n, n_atoms, (uint32_t)idx.n_types,
                         (const uint8_t*)idx.cat, (const uint32_t*)idx.arity, (const uint32_t*)idx.type,
                         (const uint64_t*)idx.tgt_off, (const uint32_t*)idx.tgt, k0, t0, t1, t2);
      DAS_HIP(hipGetLastError());
    }
    perm.alloc(R, s);
    ColSet cs{};
    cs.n = 4;
    cs.c[0] = k0; cs.c[1] = t0; cs.c[2] = t1; cs.c[3] = t2;
    sort_perm(cs, R, perm.p, std::max(27, bits_for(n_atoms)), s);
    flag.alloc(R, s);
    pos.alloc(R + 1, s);
    {
      ProfScope ps(c, "k_pc_flags", 40.0 * R);
      hipLaunchKernelGGL(k_pc_flags, G(R), dim3(kB), 0, s, (const uint32_t*)k0, (const uint32_t*)t0,
                         (const uint32_t*)t1, (const uint32_t*)t2, (const uint32_t*)perm.p, R, flag.p);
      DAS_HIP(hipGetLastError());
    }
    m = scan_total<uint32_t>(SpanIn<uint32_t>{flag.p}, R, pos.p, s);
  }
  auto out = new_table(c, DAS_TABLE_ORDERED, 7, vars, m);
  out->nrows = m;
  if (!m) return out;
  {
    const uint32_t *k0 = rows.p, *t0 = rows.p + R, *t1 = rows.p + 2 * R, *t2 = rows.p + 3 * R;
    ProfScope ps(c, "k_pc_emit", 12.0 * R + 36.0 * m);
    hipLaunchKernelGGL(k_pc_emit, G(R), dim3(kB), 0, s, k0, t0, t1, t2, (const uint32_t*)perm.p,
                       (const uint32_t*)flag.p, (const uint32_t*)pos.p, R, out->col(0), out->col(1), out->col(2),
                       out->col(3), out->col(4));
    DAS_HIP(hipGetLastError());
  }
  PcIndex X{};
  for (int p = 0; p < 2; ++p) X.p2[p] = view_of(idx.pidx[2][p], 2);
  for (int p = 0; p < 3; ++p) X.p3[p] = view_of(idx.pidx[3][p], 3);
  DBuf<uint8_t> blocked;
  upload_blocked(c, blocked);
  DBuf<unsigned long long> count(m, s);
  DBuf<uint64_t> probe(4 * m, s);                     // nch, choff, p_lo, p_len
  DBuf<uint32_t> psv(2 * m, s);                       // p_sel, p_val
  uint64_t *nch = probe.p, *choff = probe.p + m, *p_lo = probe.p + 2 * m, *p_len = probe.p + 3 * m;
  {
    // per template: its row, ~2 key searches, the probe record
    ProfScope ps(c, "k_pc_resolve", m * (20.0 + 2.0 * 8.0 * 24.0 + 48.0));
    hipLaunchKernelGGL(k_pc_resolve, G(m), dim3(kB), 0, s, m, W, (const uint32_t*)out->col(0),
                       (const uint32_t*)out->col(1), (const uint32_t*)out->col(2), (const uint32_t*)out->col(3),
                       (const uint32_t*)out->col(4), X, (const uint8_t*)blocked.p, type_named(idx, "Similarity"),
                       type_named(idx, "Set"), (const Digest*)idx.digest, count.p, nch, p_lo, p_len, psv.p,
                       psv.p + m);
    DAS_HIP(hipGetLastError());
  }
  if (X.p3[1].nkeys && X.p3[2].nkeys) {
    exclusive_scan<uint64_t>(nch, m, choff, s);
    {
      // the scope counts the probe records; the rows scanned are known on
      // the device only and are added below when profiling is on (the
      // summing scan is then timed as a scan of its own)
      ProfScope ps(c, "k_pc_scan", 40.0 * m);
      hipLaunchKernelGGL(k_pc_scan, dim3(512), dim3(kB), 0, s, m, (const uint64_t*)choff, (const uint64_t*)nch,
                         (const uint64_t*)p_lo, (const uint64_t*)p_len, (const uint32_t*)psv.p,
                         (const uint32_t*)(psv.p + m), X.p3[1].col[2], X.p3[2].col[1], count.p);
      DAS_HIP(hipGetLastError());
    }
    if (c.prof) {                                      // (profiling only: the rows read, summed on the device)
      DBuf<uint64_t> acc(m + 1, s);
      prof_add_bytes(c, "k_pc_scan", 4.0 * scan_total<uint64_t>(SpanIn<uint64_t>{p_len}, m, acc.p, s));
    }
  }
  {
    ProfScope ps(c, "k_pc_finish", 28.0 * m);
    hipLaunchKernelGGL(k_pc_finish, G(m), dim3(kB), 0, s, m, W, (const unsigned long long*)count.p, out->col(2),
                       out->col(3), out->col(4), out->col(5), out->col(6));
    DAS_HIP(hipGetLastError());
  }
  return out;
}

// ---------------------------------------------------------------------------
// conjunction counts (das_conjunction_counts): the mining loop's compute_count
// of And-combinations of templates, without a join output.  DESIGN.md §3d.
//
// A template binds V1, or (V1, V2), in wildcard order, and its rows in
// P_{a,p} are sorted by (V1[, V2]): the natural join of k of them is an
// intersection / semi-join, counted by walking one term's rows (the driver)
// and probing the others by binary search.
//   resolve  one thread per template -> CjTerm (row range, V1 / V2 columns,
//            the filter of a (1,2)-grounded template)
//   plan     one thread per combination: empty -> 0; else the driver and its
//            chunk count (kCjChunk rows each)
//   scan     exclusive scan of the chunk counts
//   count    one wave per chunk, one add per wave
// ---------------------------------------------------------------------------
namespace {

constexpr uint32_t kCjChunk = DAS_CJ_CHUNK_ROWS;          // driver rows of one wave step
constexpr uint32_t kCjCoop = 64;                          // a longer sub-range is walked by the whole wave
constexpr uint32_t kCjAllOne = 0, kCjDriveTwo = 1, kCjDriveOne = 2;   // plan modes (below)
static_assert(kCjChunk % 64 == 0, "chunks are whole waves");

struct CjTerm {
  uint64_t lo, hi;           // its rows in one P_{a,p}; empty: no such key, or a black-listed type
  const uint32_t* v1;        // the column bound to V1: ascending over [lo, hi)
  const uint32_t* v2;        // the column bound to V2: ascending inside one V1 (null: one variable)
  const uint32_t* fcol;      // targets (1,2) grounded: only the rows with fcol[r] == fval are the term's
  uint32_t fval;             //   (the rows are sorted by (v1, fcol))
  uint32_t nvars;
};

__global__ void k_cj_resolve(uint64_t m, const uint32_t* __restrict__ c_ar, const uint32_t* __restrict__ c_ty,
                             const uint32_t* __restrict__ c_t0, const uint32_t* __restrict__ c_t1,
                             const uint32_t* __restrict__ c_t2, PcIndex X, const uint8_t* __restrict__ blocked,
                             CjTerm* terms) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ar = c_ar[i], ty = c_ty[i];
    const uint32_t T[3] = {c_t0[i], c_t1[i], ar == 3 ? c_t2[i] : kNone};
    uint32_t ng = 0;
    for (uint32_t p = 0; p < ar; ++p) ng += T[p] != kNone ? 1u : 0u;
    CjTerm t{};
    t.nvars = ar - ng;
    uint64_t lo = 0, hi = 0;
    if (!(blocked && blocked[ty])) {
      if (ar == 2) {                           // [T, a, *] / [T, *, b]: the key range, V1 = the other target
        const uint32_t p = T[0] != kNone ? 0u : 1u;
        key_run(X.p2[p], ty, T[p], lo, hi);
        t.v1 = X.p2[p].col[1 - p];
      } else if (ng == 1) {                    // the key range, (V1, V2) = the other targets in position order
        const uint32_t p = T[0] != kNone ? 0u : T[1] != kNone ? 1u : 2u;
        key_run(X.p3[p], ty, T[p], lo, hi);
        t.v1 = X.p3[p].col[p == 0 ? 1 : 0];
        t.v2 = X.p3[p].col[p == 2 ? 1 : 2];
      } else if (T[2] == kNone) {              // (0,1): rows of key t0 are sorted by (t1, t2)
        if (key_run(X.p3[0], ty, T[0], lo, hi)) {
          const uint64_t a = lower_row(X.p3[0].col[1], lo, hi, T[1]);
          hi = lower_row(X.p3[0].col[1], a, hi, (uint64_t)T[1] + 1);
          lo = a;
        }
        t.v1 = X.p3[0].col[2];
      } else if (T[1] == kNone) {              // (0,2): rows of key t2 are sorted by (t0, t1)
        if (key_run(X.p3[2], ty, T[2], lo, hi)) {
          const uint64_t a = lower_row(X.p3[2].col[0], lo, hi, T[0]);
          hi = lower_row(X.p3[2].col[0], a, hi, (uint64_t)T[0] + 1);
          lo = a;
        }
        t.v1 = X.p3[2].col[1];
      } else {                                 // (1,2): the shorter key range, filtered on the other target
        uint64_t lo1, hi1, lo2, hi2;
        const bool both = key_run(X.p3[1], ty, T[1], lo1, hi1) && key_run(X.p3[2], ty, T[2], lo2, hi2);
        if (both && hi1 - lo1 <= hi2 - lo2) {
          lo = lo1; hi = hi1;
          t.v1 = X.p3[1].col[0]; t.fcol = X.p3[1].col[2]; t.fval = T[2];
        } else if (both) {
          lo = lo2; hi = hi2;
          t.v1 = X.p3[2].col[0]; t.fcol = X.p3[2].col[1]; t.fval = T[1];
        }
      }
    }
    t.lo = lo;
    t.hi = hi;
    terms[i] = t;
  }
}

// plan[c] = mode | driver << 2 | smallest two-variable term << 4 | (more than
// one two-variable term) << 6, the two terms as positions in the combination.
//   kCjAllOne    no two-variable term: drive the smallest term
//   kCjDriveTwo  drive the smallest two-variable term, probe every other term
//   kCjDriveOne  drive the smallest one-variable term (it has fewer rows than
//                any two-variable one), probe the other one-variable terms,
//                then take x's equal range in the smallest two-variable term
__global__ void k_cj_plan(uint64_t n, uint32_t k, const uint32_t* __restrict__ combo,
                          const CjTerm* __restrict__ terms, unsigned long long* count, uint64_t* nch,
                          uint64_t* drows, uint32_t* plan) {
  for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t len1 = ~0ull, len2 = ~0ull;
    uint32_t best1 = 0, best2 = 0, n1 = 0, n2 = 0;
    bool empty = false;
    for (uint32_t j = 0; j < k; ++j) {
      const CjTerm& t = terms[combo[c * k + j]];
      const uint64_t len = t.hi - t.lo;
      empty |= len == 0;
      if (t.nvars == 2) {
        ++n2;
        if (len < len2) { len2 = len; best2 = j; }
      } else {
        ++n1;
        if (len < len1) { len1 = len; best1 = j; }
      }
    }
    uint64_t rows = 0;
    uint32_t p = 0;
    if (!empty) {
      if (!n2) { rows = len1; p = kCjAllOne | best1 << 2; }
      else if (n1 && len1 < len2) { rows = len1; p = kCjDriveOne | best1 << 2 | best2 << 4 | (n2 > 1 ? 64u : 0u); }
      else { rows = len2; p = kCjDriveTwo | best2 << 2; }
    }
    count[c] = 0;
    nch[c] = (rows + kCjChunk - 1) / kCjChunk;
    drows[c] = rows;
    plan[c] = p;
  }
}

// first row of [lo, hi) with (c0, c1) >= key = c0 << 32 | c1 (rows ascending by (c0, c1))
__device__ __forceinline__ uint64_t lower_pair(const uint32_t* c0, const uint32_t* c1, uint64_t lo, uint64_t hi,
                                               uint64_t key) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((((uint64_t)c0[mid] << 32) | c1[mid]) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// is x a V1 of the one-variable term t
__device__ __forceinline__ bool cj_has1(const CjTerm& t, uint32_t x) {
  if (t.fcol) {
    const uint64_t r = lower_pair(t.v1, t.fcol, t.lo, t.hi, ((uint64_t)x << 32) | t.fval);
    return r < t.hi && t.v1[r] == x && t.fcol[r] == t.fval;
  }
  const uint64_t r = lower_row(t.v1, t.lo, t.hi, x);
  return r < t.hi && t.v1[r] == x;
}
// is (x, y) a (V1, V2) of the two-variable term t
__device__ __forceinline__ bool cj_has2(const CjTerm& t, uint32_t x, uint32_t y) {
  const uint64_t r = lower_pair(t.v1, t.v2, t.lo, t.hi, ((uint64_t)x << 32) | y);
  return r < t.hi && t.v1[r] == x && t.v2[r] == y;
}

// choff: exclusive scan of nch.  One wave per chunk of a combination's driver.
__global__ void __launch_bounds__(kB) k_cj_count(uint32_t n, uint32_t k, const uint64_t* __restrict__ choff,
                                                const uint64_t* __restrict__ nch,
                                                const uint32_t* __restrict__ combo,
                                                const uint32_t* __restrict__ plan,
                                                const CjTerm* __restrict__ terms, unsigned long long* count) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total = choff[n - 1] + nch[n - 1];
  const uint64_t nwaves = (uint64_t)gridDim.x * (kB / 64);
  for (uint64_t ch = (uint64_t)blockIdx.x * (kB / 64) + (threadIdx.x >> 6); ch < total; ch += nwaves) {
    uint32_t a = 0, b = n;                     // the last combination with choff <= ch owns the chunk
    while (a < b) {
      const uint32_t mid = a + ((b - a) >> 1);
      if (choff[mid] <= ch) a = mid + 1; else b = mid;
    }
    const uint32_t i = __builtin_amdgcn_readfirstlane(a - 1);     // one owner per wave: its records are scalar loads
    const uint32_t pl = plan[i];
    const uint32_t mode = pl & 3u, drv = (pl >> 2) & 3u, sel2 = (pl >> 4) & 3u;
    const bool several2 = (pl & 64u) != 0;
    CjTerm T[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) T[j] = terms[combo[(uint64_t)i * k + (j < k ? j : 0u)]];
    CjTerm D = T[0], S = T[0];
#pragma unroll
    for (uint32_t j = 1; j < 4; ++j) {
      if (j == drv) D = T[j];
      if (j == sel2) S = T[j];
    }
    const uint64_t r0 = D.lo + (ch - choff[i]) * kCjChunk;
    const uint64_t r1 = min(r0 + kCjChunk, D.hi);
    unsigned long long cnt = 0;
    for (uint64_t base = r0; base < r1; base += 64) {
      const uint64_t r = base + lane;
      bool ok = r < r1;
      if (ok && D.fcol) ok = D.fcol[r] == D.fval;
      uint32_t x = 0, y = 0;
      if (ok) {
        x = D.v1[r];
        if (D.nvars == 2) y = D.v2[r];
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        if (j >= k || j == drv || !ok) continue;
        if (T[j].nvars == 1) ok = cj_has1(T[j], x);
        else if (mode == kCjDriveTwo) ok = cj_has2(T[j], x, y);
      }
      if (mode != kCjDriveOne) {
        cnt += ok ? 1u : 0u;
        continue;
      }
      uint64_t sa = 0, sb = 0;                 // x's rows in the smallest two-variable term
      if (ok) {
        sa = lower_row(S.v1, S.lo, S.hi, x);
        sb = lower_row(S.v1, sa, S.hi, (uint64_t)x + 1);
      }
      if (!several2) {
        cnt += sb - sa;
        continue;
      }
      const bool wide = sb - sa > kCjCoop;
      if (!wide) {
        for (uint64_t q = sa; q < sb; ++q) {
          const uint32_t yq = S.v2[q];
          bool in = true;
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j)
            if (j < k && j != sel2 && T[j].nvars == 2 && in) in = cj_has2(T[j], x, yq);
          cnt += in ? 1u : 0u;
        }
      }
      // a hub's sub-range: the whole wave walks it, one such lane at a time
      uint64_t todo = __ballot(wide);
      while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t xl = __shfl(x, leader, 64);
        const uint64_t qa = __shfl(sa, leader, 64), qb = __shfl(sb, leader, 64);
        for (uint64_t q = qa + lane; q < qb; q += 64) {
          const uint32_t yq = S.v2[q];
          bool in = true;
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j)
            if (j < k && j != sel2 && T[j].nvars == 2 && in) in = cj_has2(T[j], xl, yq);
          cnt += in ? 1u : 0u;
        }
      }
    }
    cnt = wave_reduce_sum(cnt);
    if (lane == 0 && cnt) atomicAdd(&count[i], cnt);
  }
}

// host checks of a batch of templates (column-major arity, type, t0, t1, t2)
void cj_check_templates(const Index& idx, const uint32_t* tpl, uint64_t m) {
  const uint32_t unord[2] = {type_named(idx, "Similarity"), type_named(idx, "Set")};
  for (uint64_t i = 0; i < m; ++i) {
    const uint32_t ar = tpl[i], ty = tpl[m + i];
    DAS_CHECK(ar == 2 || ar == 3, DAS_E_INVALID, "conjunction counts: a template of arity other than 2 or 3");
    DAS_CHECK(ty < idx.n_types, DAS_E_INVALID, "conjunction counts: type id out of range");
    DAS_CHECK(ty != unord[0] && ty != unord[1], DAS_E_UNSUPPORTED,
              "conjunction counts: Similarity / Set templates take the per-query path");
    uint32_t ng = 0;
    for (uint32_t p = 0; p < ar; ++p) {
      const uint32_t t = tpl[(2 + p) * m + i];
      if (t == kNone) continue;
      DAS_CHECK(t < idx.n_atoms, DAS_E_INVALID, "conjunction counts: grounded target out of range");
      ++ng;
    }
    DAS_CHECK(ng >= 1 && ng < ar, DAS_E_INVALID, "conjunction counts: a template needs a wildcard and a grounded target");
  }
}

// terms[i] = the descriptor of host template i (checked): one upload, one launch
void cj_resolve(Ctx& c, const uint32_t* tpl, uint64_t m, DBuf<CjTerm>& terms) {
  const Index& idx = c.idx;
  hipStream_t s = c.s;
  terms.alloc(m, s);
  DBuf<uint32_t> d_tpl(5 * m, s);
  DBuf<uint8_t> blocked;
  upload_blocked(c, blocked);
  DAS_HIP(hipMemcpyAsync(d_tpl.p, tpl, 20 * m, hipMemcpyHostToDevice, s));
  PcIndex X{};
  for (int p = 0; p < 2; ++p) X.p2[p] = view_of(idx.pidx[2][p], 2);
  for (int p = 0; p < 3; ++p) X.p3[p] = view_of(idx.pidx[3][p], 3);
  // per template: its row, ~2 key searches and an equal range -- a rough bound of 3 searches of
  // 24 steps, every step taken as an 8-byte ukey word (an equal range's steps read 4-byte column
  // words) -- and the descriptor
  ProfScope ps(c, "k_cj_resolve", m * (20.0 + 3.0 * 8.0 * 24.0 + sizeof(CjTerm)));
  hipLaunchKernelGGL(k_cj_resolve, G(m), dim3(kB), 0, s, m, (const uint32_t*)d_tpl.p,
                     (const uint32_t*)(d_tpl.p + m), (const uint32_t*)(d_tpl.p + 2 * m),
                     (const uint32_t*)(d_tpl.p + 3 * m), (const uint32_t*)(d_tpl.p + 4 * m), X,
                     (const uint8_t*)blocked.p, terms.p);
  DAS_HIP(hipGetLastError());
}

// d_count[r] = the count of device row r of d_combo (k indices into terms),
// 0 < n < 2^32: plan, scan, count; nothing is read back
void cj_count_rows(Ctx& c, const CjTerm* terms, const uint32_t* d_combo, uint64_t n, uint32_t k,
                   unsigned long long* d_count) {
  hipStream_t s = c.s;
  DBuf<uint32_t> plan(n, s);
  DBuf<uint64_t> ch(3 * n, s);                        // nch, choff, driver rows
  {
    ProfScope ps(c, "k_cj_plan", n * (k * (4.0 + 24.0) + 28.0));
    hipLaunchKernelGGL(k_cj_plan, G(n), dim3(kB), 0, s, n, k, d_combo, terms, d_count, ch.p, ch.p + 2 * n, plan.p);
    DAS_HIP(hipGetLastError());
  }
  exclusive_scan<uint64_t>(ch.p, n, ch.p + n, s);
  {
    // The scope counts the combinations' records; the driver rows walked are
    // known on the device only and are added below when profiling is on.  The
    // probes (~log2(range) dependent loads per row and other term, through
    // L2 / MALL) are not bytes of a stream and are not counted: the kernel
    // is bound by their latency, not by HBM.
    ProfScope ps(c, "k_cj_count", n * (16.0 + 4.0 + k * (4.0 + sizeof(CjTerm)) + 8.0));
    hipLaunchKernelGGL(k_cj_count, dim3(2048), dim3(kB), 0, s, (uint32_t)n, k, (const uint64_t*)(ch.p + n),
                       (const uint64_t*)ch.p, d_combo, (const uint32_t*)plan.p, terms, d_count);
    DAS_HIP(hipGetLastError());
  }
  if (c.prof) {                                        // (profiling only: the driver rows, summed on the device)
    DBuf<uint64_t> acc(n + 1, s);
    prof_add_bytes(c, "k_cj_count", 4.0 * scan_total<uint64_t>(SpanIn<uint64_t>{ch.p + 2 * n}, n, acc.p, s));
  }
}

}  // namespace

void conjunction_counts(Ctx& c, const uint32_t* tpl, uint64_t m, const uint32_t* combo, uint64_t n, uint32_t k,
                        uint64_t* counts) {
  DAS_CHECK(k >= 2 && k <= 4, DAS_E_INVALID, "conjunction counts: k outside 2..4");
  miner_check(c);
  DAS_CHECK((tpl || !m) && (combo || !n) && (counts || !n), DAS_E_INVALID, "conjunction counts: null argument");
  DAS_CHECK(m < (1ull << 32) && n < (1ull << 32), DAS_E_UNSUPPORTED, "conjunction counts: too many rows in one call");
  cj_check_templates(c.idx, tpl, m);
  for (uint64_t i = 0; i < n * k; ++i)
    DAS_CHECK(combo[i] < m, DAS_E_INVALID, "conjunction counts: template index out of range");
  if (!n) return;
  hipStream_t s = c.s;
  DBuf<uint32_t> d_combo(n * k, s);
  DBuf<CjTerm> terms;
  DBuf<unsigned long long> count(n, s);
  DAS_HIP(hipMemcpyAsync(d_combo.p, combo, 4 * n * k, hipMemcpyHostToDevice, s));
  cj_resolve(c, tpl, m, terms);
  cj_count_rows(c, terms.p, d_combo.p, n, k, count.p);
  DAS_HIP(hipMemcpyAsync(counts, count.p, 8 * n, hipMemcpyDeviceToHost, s));
  DAS_HIP(hipStreamSynchronize(s));
  count_readback();
}

// ---------------------------------------------------------------------------
// exhaustive search (das_mine_combinations): the notebook's last cell (efac9ac6)
// for ngram 2 and 3 -- every basic with every ascending (k - 1)-tuple of
// candidates, counted, scored (compute_isurprisingness) and cut to the best
// `top`, without a combination crossing the bus.  DESIGN.md §3d.
//   pair matrix  count(b, c) of every basic x candidate, rows made on the device
//   partners     per basic the candidates with count > 0 (not b itself), in
//                order, each with its pair count; one read-back of the sizes
//   tiles        DAS_MX_TILE ranks of sum_b C(|S_b|, 2): rank -> (b, i, j)
//                (mx_unrank.h), the triples and their (i, j) pairs counted by
//                the plan / scan / count above, scored, the survivors
//                compacted in rank order behind the running top rows, and the
//                lot stable-sorted by value, descending, and cut
// A triple outside the partner lists has a pair count of 0 and so the value 0
// (or nan): it cannot be reported.  k = 2 scores the pair matrix itself.
// ---------------------------------------------------------------------------
namespace {

__global__ void k_mx_pair_rows(uint64_t r0, uint64_t n, uint64_t nc, const uint32_t* __restrict__ basics,
                               const uint32_t* __restrict__ cands, uint32_t* combo) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = r0 + t;
    combo[2 * t] = basics[r / nc];
    combo[2 * t + 1] = cands[r % nc];
  }
}

// 1: candidate r % nc is a partner of basic r / nc
struct MxPartnerIn {
  const unsigned long long* pcount;
  const uint32_t* basics;
  const uint32_t* cands;
  uint64_t nc;
  __device__ __forceinline__ uint32_t operator()(uint64_t r) const {
    return pcount[r] > 0 && cands[r % nc] != basics[r / nc] ? 1u : 0u;
  }
  static std::string name() { return "MxPartnerIn"; }
};

// pos: exclusive scan of the partner flags over the n2 = nb * nc matrix rows.
// part_tpl / part_cnt: the partners of basic 0, of basic 1, .. in candidate
// order; s_off[b] = where basic b's begin, s_off[nb] = their number.
__global__ void k_mx_partners(uint64_t n2, uint64_t nb, MxPartnerIn in, const uint32_t* __restrict__ pos,
                              uint32_t* part_tpl, unsigned long long* part_cnt, uint64_t* s_off) {
  for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n2; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t f = in(r), o = pos[r];
    if (f) {
      part_tpl[o] = in.cands[r % in.nc];
      part_cnt[o] = in.pcount[r];
    }
    if (r % in.nc == 0) s_off[r / in.nc] = o;
    if (r == n2 - 1) s_off[nb] = (uint64_t)o + f;
  }
}

// Ranks [g0, g0 + n) -> rows: pre[b] = the triangles of the basics before b
// (pre[nb] = all), so the last b with pre[b] <= g owns rank g.
// aux: where the row's two partners sit in part_tpl / part_cnt.
__global__ void k_mx_enum(uint64_t g0, uint64_t n, uint32_t nb, const uint64_t* __restrict__ pre,
                          const uint64_t* __restrict__ s_off, const uint32_t* __restrict__ basics,
                          const uint32_t* __restrict__ part_tpl, uint32_t* combo3, uint32_t* combo2, uint32_t* aux) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = g0 + t;
    uint32_t a = 0, e = nb;
    while (a < e) {
      const uint32_t mid = a + ((e - a) >> 1);
      if (pre[mid] <= g) a = mid + 1; else e = mid;
    }
    const uint32_t b = a - 1;                          // pre[0] = 0 <= g: a >= 1; pre[b + 1] > g: s >= 2
    const uint64_t base = s_off[b], s = s_off[b + 1] - base;
    uint32_t i, j;
    mx_unrank(g - pre[b], s, i, j);
    const uint32_t ti = part_tpl[base + i], tj = part_tpl[base + j];
    combo3[3 * t] = basics[b];
    combo3[3 * t + 1] = ti;
    combo3[3 * t + 2] = tj;
    combo2[2 * t] = ti;
    combo2[2 * t + 1] = tj;
    aux[2 * t] = (uint32_t)(base + i);
    aux[2 * t + 1] = (uint32_t)(base + j);
  }
}

// compute_isurprisingness in float64 and in the notebook's order of
// operations (miner.isurprisingness_from_counts is matched bit for bit): IEEE
// division and multiplication, each rounded once -- contraction is off for
// this function, so no product is fused into the subtraction after it.
__device__ __forceinline__ double mx_value(uint32_t k, double u, unsigned long long c, const unsigned long long tc[3],
                                           const unsigned long long pc[3], bool normalized) {
#pragma clang fp contract(off)
  const double p = (double)c / u;
  const double t0 = (double)tc[0] / u, t1 = (double)tc[1] / u;
  double mx, mn;
  if (k == 2) {
    mx = mn = t0 * t1;
  } else {
    const double t2 = (double)tc[2] / u;
    const double s0 = (t0 * t1) * t2;
    const double s1 = ((double)pc[0] / u) * t2;
    const double s2 = ((double)pc[1] / u) * t1;
    const double s3 = ((double)pc[2] / u) * t0;
    mx = fmax(fmax(s0, s1), fmax(s2, s3));
    mn = fmin(fmin(s0, s1), fmin(s2, s3));
  }
  const double hi = p - mx, lo = mn - p;
  double v = fmax(hi, lo);
  if (normalized) v = p > 0 ? v / p : __builtin_nan("");
  return v;
}

// value[t] and flag[t] (1: reported unless cut) of the tile's n rows.  k = 3:
// cnt2 = the counts of the (i, j) pairs, aux as k_mx_enum wrote it.
__global__ void k_mx_score(uint64_t n, uint32_t k, const uint32_t* __restrict__ combo,
                           const unsigned long long* __restrict__ tcount, const unsigned long long* __restrict__ cnt,
                           const unsigned long long* __restrict__ cnt2, const uint32_t* __restrict__ aux,
                           const unsigned long long* __restrict__ part_cnt, double u, unsigned long long support,
                           uint32_t normalized, double* value, uint32_t* flag) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
    unsigned long long tc[3] = {0, 0, 0}, pc[3] = {0, 0, 0};
    bool valid = true;
    if (k == 2) {
      const uint32_t b = combo[2 * t], d = combo[2 * t + 1];
      tc[0] = tcount[b];
      tc[1] = tcount[d];
      valid = b != d;                                  // a basic is never inside its own tuple
    } else {
      for (uint32_t j = 0; j < 3; ++j) tc[j] = tcount[combo[3 * t + j]];
      pc[0] = part_cnt[aux[2 * t]];
      pc[1] = part_cnt[aux[2 * t + 1]];
      pc[2] = cnt2[t];
    }
    const unsigned long long c = cnt[t];
    const double v = mx_value(k, u, c, tc, pc, normalized != 0);
    value[t] = v;
    flag[t] = valid && v > 0 && c >= support ? 1u : 0u;
  }
}

// the tile's flagged rows, in rank order, behind the `at` rows kept so far
__global__ void k_mx_emit(uint64_t n, uint32_t k, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                          const uint32_t* __restrict__ combo, const unsigned long long* __restrict__ cnt,
                          const double* __restrict__ value, uint64_t at, uint32_t* s_combo, unsigned long long* s_cnt,
                          double* s_val) {
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
    if (!flag[t]) continue;
    const uint64_t o = at + pos[t];
    for (uint32_t j = 0; j < k; ++j) s_combo[o * k + j] = combo[t * k + j];
    s_cnt[o] = cnt[t];
    s_val[o] = value[t];
  }
}

// a positive double orders as its bits: the complement sorts descending
__global__ void k_mx_keys(uint64_t n, const double* __restrict__ s_val, uint32_t* key_hi, uint32_t* key_lo) {
  for (uint64_t o = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; o < n; o += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long bits = ~(unsigned long long)__double_as_longlong(s_val[o]);
    key_hi[o] = (uint32_t)(bits >> 32);
    key_lo[o] = (uint32_t)bits;
  }
}

__global__ void k_mx_take(uint64_t n, uint32_t k, const uint32_t* __restrict__ perm,
                          const uint32_t* __restrict__ a_combo, const unsigned long long* __restrict__ a_cnt, const double* __restrict__ a_val,
                          uint32_t* b_combo, unsigned long long* b_cnt, double* b_val) {
  for (uint64_t o = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; o < n; o += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = perm[o];
    for (uint32_t j = 0; j < k; ++j) b_combo[o * k + j] = a_combo[r * k + j];
    b_cnt[o] = a_cnt[r];
    b_val[o] = a_val[r];
  }
}

struct MxSel {                                         // kept rows: the running top, then a tile's survivors
  DBuf<uint32_t> combo;
  DBuf<unsigned long long> cnt;
  DBuf<double> val;
  void alloc(uint64_t rows, uint32_t k, hipStream_t s) {
    combo.alloc(rows * k, s);
    cnt.alloc(rows, s);
    val.alloc(rows, s);
  }
};

uint64_t mx_tile() {
  const long long t = env_int("DAS_MX_TILE", DAS_MX_TILE);
  return (uint64_t)std::max(1ll, std::min(t, 1ll << 28));
}

}  // namespace

void mine_combinations(Ctx& c, const uint32_t* tpl, uint64_t m, const uint64_t* tpl_count, const uint32_t* basics,
                       uint64_t nb, const uint32_t* cands, uint64_t nc, uint32_t k, uint64_t universe_size,
                       uint64_t support, bool normalized, uint32_t top, uint64_t max_combinations,
                       uint32_t* out_combo, uint64_t* out_count, double* out_value, uint32_t* n_out,
                       uint64_t stats[3]) {
  DAS_CHECK(k == 2 || k == 3, DAS_E_INVALID, "mine: k outside 2..3");
  miner_check(c);
  DAS_CHECK((tpl || !m) && (tpl_count || !m) && (basics || !nb) && (cands || !nc) && out_combo && out_count &&
                out_value && n_out && stats,
            DAS_E_INVALID, "mine: null argument");
  DAS_CHECK(top >= 1 && top <= DAS_MX_MAX_TOP, DAS_E_INVALID, "mine: top outside 1..DAS_MX_MAX_TOP");
  DAS_CHECK(universe_size > 0, DAS_E_INVALID, "mine: universe size 0");
  DAS_CHECK(m < (1ull << 32), DAS_E_UNSUPPORTED, "mine: too many templates in one call");
  cj_check_templates(c.idx, tpl, m);
  std::vector<uint8_t> seen(m, 0);                     // bit 0: a basic, bit 1: a candidate
  for (uint64_t i = 0; i < nb; ++i) {
    DAS_CHECK(basics[i] < m, DAS_E_INVALID, "mine: template index out of range");
    DAS_CHECK(!(seen[basics[i]] & 1), DAS_E_INVALID, "mine: a basic twice");
    seen[basics[i]] |= 1;
  }
  for (uint64_t i = 0; i < nc; ++i) {
    DAS_CHECK(cands[i] < m, DAS_E_INVALID, "mine: template index out of range");
    DAS_CHECK(!(seen[cands[i]] & 2), DAS_E_INVALID, "mine: a candidate twice");
    seen[cands[i]] |= 2;
  }
  DAS_CHECK(nb * nc < (1ull << 32), DAS_E_UNSUPPORTED, "mine: basics x candidates of 2^32 pairs or more");
  uint64_t searched = 0;                               // the space as defined: < nb nc^2 / 2 < 2^63
  for (uint64_t i = 0; i < nb; ++i) {
    const uint64_t av = nc - (seen[basics[i]] & 2 ? 1 : 0);
    searched += k == 2 ? av : av >= 2 ? mx_pairs(av) : 0;
  }
  *n_out = 0;
  stats[0] = searched;
  stats[1] = stats[2] = 0;
  const uint64_t n2 = nb * nc;
  if (!n2) return;
  stats[1] = n2;
  DAS_CHECK(n2 <= max_combinations, DAS_E_LIMIT,
            "mine: " + std::to_string(n2) + " combinations to score, more than max_combinations");

  hipStream_t s = c.s;
  const uint64_t tile = mx_tile();
  DBuf<CjTerm> terms;
  cj_resolve(c, tpl, m, terms);
  DBuf<unsigned long long> tcount(m, s), pcount(n2, s);
  DBuf<uint32_t> ids(nb + nc, s);
  DAS_HIP(hipMemcpyAsync(tcount.p, tpl_count, 8 * m, hipMemcpyHostToDevice, s));
  DAS_HIP(hipMemcpyAsync(ids.p, basics, 4 * nb, hipMemcpyHostToDevice, s));
  DAS_HIP(hipMemcpyAsync(ids.p + nb, cands, 4 * nc, hipMemcpyHostToDevice, s));
  const uint32_t *d_basics = ids.p, *d_cands = ids.p + nb;

  // the pair matrix, a tile of rows at a time
  DBuf<uint32_t> combo(3 * std::min(tile, n2), s);
  for (uint64_t r0 = 0; r0 < n2; r0 += tile) {
    const uint64_t n = std::min(tile, n2 - r0);
    {
      ProfScope ps(c, "k_mx_pair_rows", 16.0 * n);
      hipLaunchKernelGGL(k_mx_pair_rows, G(n), dim3(kB), 0, s, r0, n, nc, d_basics, d_cands, combo.p);
      DAS_HIP(hipGetLastError());
    }
    cj_count_rows(c, terms.p, combo.p, n, 2, pcount.p + r0);
  }

  // the partner lists and the ranks of the triples
  DBuf<uint32_t> part_tpl;
  DBuf<unsigned long long> part_cnt;
  DBuf<uint64_t> offs;                                 // s_off[nb + 1], pre[nb + 1]
  std::vector<uint64_t> h_pre(nb + 1, 0);              // (uploaded below: lives to the end of the call)
  uint64_t total = n2;                                 // ranks to score: k = 2, the matrix rows
  if (k == 3) {
    const MxPartnerIn in{pcount.p, d_basics, d_cands, nc};
    DBuf<uint32_t> pos(n2, s);
    exclusive_scan_fn<uint32_t>(in, n2, pos.p, s);
    part_tpl.alloc(n2, s);
    part_cnt.alloc(n2, s);
    offs.alloc(2 * (nb + 1), s);
    {
      ProfScope ps(c, "k_mx_partners", n2 * (8.0 + 4.0 + 4.0 + 12.0) + 8.0 * (nb + 1));
      hipLaunchKernelGGL(k_mx_partners, G(n2), dim3(kB), 0, s, n2, nb, in, (const uint32_t*)pos.p, part_tpl.p,
                         part_cnt.p, offs.p);
      DAS_HIP(hipGetLastError());
    }
    std::vector<uint64_t> h_off(nb + 1);
    DAS_HIP(hipMemcpyAsync(h_off.data(), offs.p, 8 * (nb + 1), hipMemcpyDeviceToHost, s));
    DAS_HIP(hipStreamSynchronize(s));
    count_readback();
    for (uint64_t b = 0; b < nb; ++b) {
      DAS_CHECK(h_off[b] <= h_off[b + 1] && h_off[b + 1] - h_off[b] <= nc, DAS_E_INTERNAL,
                "mine: partner list out of range");
      h_pre[b + 1] = h_pre[b] + mx_pairs(h_off[b + 1] - h_off[b]);      // the lists are disjoint parts of n2 < 2^32
    }
    total = h_pre[nb];
    stats[1] = n2 + total;
    DAS_CHECK(stats[1] <= max_combinations, DAS_E_LIMIT,
              "mine: " + std::to_string(stats[1]) + " combinations to score, more than max_combinations");
    DAS_HIP(hipMemcpyAsync(offs.p + nb + 1, h_pre.data(), 8 * (nb + 1), hipMemcpyHostToDevice, s));
  }

  // tiles of ranks: count, score, keep the best `top`
  const uint64_t tn = std::min(tile, std::max<uint64_t>(total, 1));
  DBuf<uint32_t> combo2, aux, flag(tn, s), pos(tn + 1, s), keys, perm;
  DBuf<unsigned long long> cnt3, cnt2;
  DBuf<double> value(tn, s);
  if (k == 3) {
    if (combo.n < 3 * tn) combo.alloc(3 * tn, s);
    combo2.alloc(2 * tn, s);
    aux.alloc(2 * tn, s);
    cnt3.alloc(tn, s);
    cnt2.alloc(tn, s);
  }
  MxSel sel[2];
  sel[0].alloc(top + tn, k, s);
  sel[1].alloc(top + tn, k, s);
  keys.alloc(2 * (top + tn), s);
  perm.alloc(top + tn, s);
  const double u = (double)universe_size;
  uint64_t kept = 0, tiles = 0;
  int cur = 0;
  for (uint64_t g0 = 0; g0 < total; g0 += tile, ++tiles) {
    const uint64_t n = std::min(tile, total - g0);
    const unsigned long long* cnt = nullptr;
    if (k == 2) {
      ProfScope ps(c, "k_mx_pair_rows", 16.0 * n);
      hipLaunchKernelGGL(k_mx_pair_rows, G(n), dim3(kB), 0, s, g0, n, nc, d_basics, d_cands, combo.p);
      DAS_HIP(hipGetLastError());
      cnt = pcount.p + g0;
    } else {
      {
        // per rank: ~log2(nb) prefix words, two offsets, two partner ids; the rows written
        ProfScope ps(c, "k_mx_enum", n * (8.0 * 4.0 + 16.0 + 8.0 + 12.0 + 8.0 + 8.0));
        hipLaunchKernelGGL(k_mx_enum, G(n), dim3(kB), 0, s, g0, n, (uint32_t)nb, (const uint64_t*)(offs.p + nb + 1),
                           (const uint64_t*)offs.p, d_basics, (const uint32_t*)part_tpl.p, combo.p, combo2.p, aux.p);
        DAS_HIP(hipGetLastError());
      }
      cj_count_rows(c, terms.p, combo.p, n, 3, cnt3.p);
      cj_count_rows(c, terms.p, combo2.p, n, 2, cnt2.p);
      cnt = cnt3.p;
    }
    {
      // per row: its indices, the terms' counts, its own and the pair counts; value and flag
      ProfScope ps(c, "k_mx_score", n * (4.0 * k + 8.0 * k + 8.0 + (k == 3 ? 8.0 + 24.0 : 0.0) + 12.0));
      hipLaunchKernelGGL(k_mx_score, G(n), dim3(kB), 0, s, n, k, (const uint32_t*)combo.p,
                         (const unsigned long long*)tcount.p, cnt, (const unsigned long long*)cnt2.p,
                         (const uint32_t*)aux.p, (const unsigned long long*)part_cnt.p, u,
                         (unsigned long long)support, normalized ? 1u : 0u, value.p, flag.p);
      DAS_HIP(hipGetLastError());
    }
    const uint64_t ns = scan_total<uint32_t>(SpanIn<uint32_t>{flag.p}, n, pos.p, s);   // the tile's read-back
    DAS_CHECK(ns <= n, DAS_E_INTERNAL, "mine: more survivors than rows");
    if (!ns) continue;
    MxSel &A = sel[cur], &B = sel[cur ^ 1];
    {
      ProfScope ps(c, "k_mx_emit", 8.0 * n + ns * (4.0 * k + 16.0) * 2.0);
      hipLaunchKernelGGL(k_mx_emit, G(n), dim3(kB), 0, s, n, k, (const uint32_t*)flag.p, (const uint32_t*)pos.p,
                         (const uint32_t*)combo.p, cnt, (const double*)value.p, kept, A.combo.p, A.cnt.p, A.val.p);
      DAS_HIP(hipGetLastError());
    }
    const uint64_t have = kept + ns, take = std::min<uint64_t>(have, top);
    {
      ProfScope ps(c, "k_mx_keys", 16.0 * have);
      hipLaunchKernelGGL(k_mx_keys, G(have), dim3(kB), 0, s, have, (const double*)A.val.p, keys.p, keys.p + have);
      DAS_HIP(hipGetLastError());
    }
    ColSet cs{};
    cs.n = 2;
    cs.c[0] = keys.p;
    cs.c[1] = keys.p + have;
    sort_perm(cs, have, perm.p, 32, s);
    {
      ProfScope ps(c, "k_mx_take", take * (4.0 + (4.0 * k + 16.0) * 2.0));
      hipLaunchKernelGGL(k_mx_take, G(take), dim3(kB), 0, s, take, k, (const uint32_t*)perm.p,
                         (const uint32_t*)A.combo.p, (const unsigned long long*)A.cnt.p, (const double*)A.val.p,
                         B.combo.p, B.cnt.p, B.val.p);
      DAS_HIP(hipGetLastError());
    }
    kept = take;
    cur ^= 1;
  }
  stats[2] = tiles;
  *n_out = (uint32_t)kept;
  if (kept) {
    const MxSel& A = sel[cur];
    DAS_HIP(hipMemcpyAsync(out_combo, A.combo.p, 4 * kept * k, hipMemcpyDeviceToHost, s));
    DAS_HIP(hipMemcpyAsync(out_count, A.cnt.p, 8 * kept, hipMemcpyDeviceToHost, s));
    DAS_HIP(hipMemcpyAsync(out_value, A.val.p, 8 * kept, hipMemcpyDeviceToHost, s));
  }
  DAS_HIP(hipStreamSynchronize(s));                    // also before the buffers above go back to the allocator
  count_readback();
}

}  // namespace das
