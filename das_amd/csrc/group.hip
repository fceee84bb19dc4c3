// Rows of an answer per value of one variable (das_group_counts, DESIGN.md
// §3f).  Every input is a key column with a weight per row; unresolved tables
// are counted from what they keep:
//   resolved / VIEW  the column, weight 1
//   PRODUCT          the factor's column, weight = the other factor's rows
//   EXPAND           the probe column, weight = the probe row's index rows
//                    (a fresh variable of the expansion: settled, weight 1)
// Two strategies accumulate into 64-bit counters: direct-address bins over the
// columns' host-known bounds (LDS bins per workgroup where the range fits a
// tile), or a sort of the keys with a run sum.  One pass then compacts the
// non-zero counters to (id ascending, count).
#include "das_internal.h"
#include "group_plan.h"

namespace das {
namespace {

constexpr int B = 256;

struct GroupSrc {
  const uint32_t* key;
  const uint32_t* rowid;   // with lc: the row's entry of lc
  const uint2* lc;         // non-null: weight = lc[rowid[i]].y
  uint64_t n;
  uint64_t w;              // lc null: every row's weight
};

__device__ __forceinline__ uint64_t src_weight(const GroupSrc& s, uint64_t i) {
  return s.lc ? (uint64_t)s.lc[s.rowid[i]].y : s.w;
}

// Adds w at bins[d] for every lane with d != kNone, a run of equal d in
// consecutive lanes as one add by its first lane (sorted keys: one add per
// key and wave; a hub key filling the wave: one add).  Call wave-uniformly.
__device__ __forceinline__ void wave_run_add(uint32_t d, uint64_t w, uint64_t* bins) {
  const int lane = __lane_id();
  const uint32_t dp = __shfl_up(d, 1, 64);
  const bool head = lane == 0 || dp != d;
  const uint64_t heads = __ballot(head);
  uint64_t sum = w;
  if (heads != ~0ull) {
    const uint64_t incl = wave_inclusive_scan<uint64_t>(w);
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int last = above ? lane + __ffsll((unsigned long long)above) - 1 : 63;   // the run's last lane
    sum = __shfl(incl, last, 64) - (incl - w);
  }
  if (head && d != kNone && sum) atomicAdd(reinterpret_cast<unsigned long long*>(bins) + d, (unsigned long long)sum);
}

// bins[key - lo] += weight over the rows of `s`.  kLds: the workgroup counts
// into LDS bins (range <= kGroupLdsBins) and adds its non-zero bins to the
// global ones afterwards, consecutive lanes on consecutive bins.  A key outside
// [lo, lo + range) is counted in *oob and left out (the bounds are the
// caller's claim; nothing is written out of range).
template <bool kLds>
__global__ void __launch_bounds__(B) k_group_accum(GroupSrc s, uint32_t lo, uint32_t range, uint64_t* bins,
                                                   uint32_t* oob) {
  __shared__ uint64_t s_bins[kLds ? kGroupLdsBins : 1];
  if (kLds) {
    for (uint32_t i = threadIdx.x; i < range; i += B) s_bins[i] = 0;
    __syncthreads();
  }
  const uint64_t stride = (uint64_t)gridDim.x * B;
  const uint64_t rounds = (s.n + stride - 1) / stride;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + (uint64_t)blockIdx.x * B + threadIdx.x;
    uint32_t d = kNone;
    uint64_t w = 0;
    if (i < s.n) {
      w = src_weight(s, i);
      d = s.key[i] - lo;
      if (d >= range) {
        if (w) atomicAdd(oob, 1u);
        d = kNone;
        w = 0;
      }
    }
    wave_run_add(d, w, kLds ? s_bins : bins);
  }
  if (kLds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < range; i += B) {
      const uint64_t v = s_bins[i];
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(bins) + i, (unsigned long long)v);
    }
  }
}

// the sorted strategy's input: every source's keys and weights back to back
__global__ void __launch_bounds__(B) k_group_pack(GroupSrc s, uint32_t* key, uint64_t* w) {
  for (uint64_t i = blockIdx.x * (uint64_t)B + threadIdx.x; i < s.n; i += (uint64_t)gridDim.x * B) {
    key[i] = s.key[i];
    w[i] = src_weight(s, i);
  }
}

// 1 where row i of the sorted order begins a run of equal keys
struct HeadIn {
  const uint32_t* key;
  const uint32_t* perm;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    return i == 0 || key[perm[i]] != key[perm[i - 1]] ? 1u : 0u;
  }
};

// run r (= off[i + 1] - 1, off the exclusive scan of the heads) of the sorted
// order: bins[r] += weight, run_key[r] = the key
__global__ void __launch_bounds__(B) k_group_runs(const uint32_t* key, const uint64_t* w, const uint32_t* perm,
                                                  const uint32_t* off, uint64_t n, uint64_t* bins,
                                                  uint32_t* run_key) {
  const uint64_t stride = (uint64_t)gridDim.x * B;
  const uint64_t rounds = (n + stride - 1) / stride;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + (uint64_t)blockIdx.x * B + threadIdx.x;
    uint32_t d = kNone;
    uint64_t wt = 0;
    if (i < n) {
      const uint32_t p = perm[i];
      d = off[i + 1] - 1u;
      wt = w[p];
      if (off[i + 1] != off[i]) run_key[d] = key[p];
    }
    wave_run_add(d, wt, bins);
  }
}

struct NzIn {
  const uint64_t* bins;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return bins[i] ? 1u : 0u; }
};

// non-zero bins to (id, count) at their exclusive offsets; bin_id null: id = lo + bin
__global__ void __launch_bounds__(B) k_group_compact(const uint64_t* bins, const uint32_t* bin_id, uint32_t lo,
                                                     uint64_t nbins, const uint32_t* off, uint32_t* ids,
                                                     uint64_t* counts) {
  for (uint64_t i = blockIdx.x * (uint64_t)B + threadIdx.x; i < nbins; i += (uint64_t)gridDim.x * B) {
    const uint64_t v = bins[i];
    if (v) {
      const uint32_t o = off[i];
      ids[o] = bin_id ? bin_id[i] : lo + (uint32_t)i;
      counts[o] = v;
    }
  }
}

// bins (+ their ids) -> c.group
uint64_t compact_bins(Ctx& c, const uint64_t* bins, const uint32_t* bin_id, uint32_t lo, uint64_t nbins) {
  DBuf<uint32_t> off(nbins + 1, c.s);
  uint64_t total;
  {
    ProfScope ps(c, "k_group_scan", 8.0 * nbins + 4.0 * nbins);
    total = scan_total<uint32_t>(NzIn{bins}, nbins, off.p, c.s);
  }
  c.group.ids.alloc(total ? total : 1, c.s);
  c.group.counts.alloc(total ? total : 1, c.s);
  if (total) {
    ProfScope ps(c, "k_group_compact", 8.0 * nbins + 4.0 * nbins + 12.0 * total);
    hipLaunchKernelGGL(k_group_compact, dim3(grid_for(nbins, B, 8192)), dim3(B), 0, c.s, bins, bin_id, lo, nbins,
                       (const uint32_t*)off.p, c.group.ids.p, c.group.counts.p);
    DAS_HIP(hipGetLastError());
  }
  return total;
}

double src_bytes(const GroupSrc& s) { return (s.lc ? 16.0 : 4.0) * s.n; }

}  // namespace

uint64_t group_counts(Ctx& c, Table* const* ts, const int32_t* cols, uint32_t n, uint64_t stats[2]) {
  std::vector<GroupSrc> src;
  uint64_t rows = 0;                       // input rows read (a product's: one factor's)
  uint32_t lo = kNone, hi = 0;
  bool bounded = true;
  for (uint32_t i = 0; i < n; ++i) {
    Table& t = *ts[i];
    const int col = cols[i];
    DAS_CHECK(t.kind == DAS_TABLE_ORDERED, DAS_E_INVALID, "group counts of a table that is not ORDERED");
    DAS_CHECK(col >= 0 && col < t.ncols, DAS_E_INVALID, "bad column");
    if (t.lazy)
      DAS_CHECK(!t.lazy->aliases_index() || t.lazy->ctx == &c, DAS_E_INVALID,
                "an unresolved answer is read through the context that made it");
    GroupSrc s{nullptr, nullptr, nullptr, 0, 1};
    if (t.lazy && t.lazy->kind == Lazy::EXPAND) {
      ExpansionCol e;
      if (expansion_probe_col(t, col, e)) {
        s = GroupSrc{e.key, e.rowid, e.lc, e.n, 0};
        stats[0]++;
      } else {
        settle(c, t);
        stats[1]++;
      }
    }
    if (t.lazy && t.lazy->kind == Lazy::PRODUCT) {
      const Lazy& r = *t.lazy;
      s = r.side[col] ? GroupSrc{r.bcol(r.src[col]), nullptr, nullptr, r.nb, r.np}
                      : GroupSrc{r.pcol(r.src[col]), nullptr, nullptr, r.np, r.nb};
      stats[0]++;
    } else if (t.lazy && t.lazy->kind == Lazy::VIEW) {
      s = GroupSrc{t.data + (uint64_t)col * t.cap, nullptr, nullptr, t.nrows, 1};
      stats[0]++;
    } else if (!t.lazy) {
      s = GroupSrc{t.col(col), nullptr, nullptr, t.nrows, 1};
    }
    if (!s.n || (!s.lc && !s.w)) continue;
    src.push_back(s);
    rows += s.n;
    if (t.lo[col] == 0 && t.hi[col] == kNone) bounded = false;
    lo = std::min(lo, t.lo[col]);
    hi = std::max(hi, t.hi[col]);
  }
  c.group.valid = false;
  c.group.n = 0;
  if (src.empty()) return 0;
  if (!bounded) {
    // [0, n_atoms) where a bound is unknown
    lo = 0;
    hi = c.idx.built && c.idx.n_atoms ? (uint32_t)(c.idx.n_atoms - 1) : kNone;
  }
  DAS_CHECK(lo <= hi, DAS_E_INTERNAL, "group counts: empty column bounds of a table with rows");
  const uint64_t range = (uint64_t)hi - lo + 1;
  const GroupPlan plan = group_plan(range, rows, env_char("DAS_GROUP_DIRECT"));
  DAS_CHECK(plan != GROUP_NONE, DAS_E_LIMIT, "group counts: key range and row count both beyond the limits");

  DBuf<uint32_t> oob(1, c.s);
  fill_dev(oob.p, 0, 4, c.s);
  uint64_t total = 0;
  if (plan == GROUP_SORTED) {
    DBuf<uint32_t> key(rows, c.s), perm(rows, c.s), off(rows + 1, c.s);
    DBuf<uint64_t> w(rows, c.s);
    uint64_t at = 0;
    for (const GroupSrc& s : src) {
      ProfScope ps(c, "k_group_pack", src_bytes(s) + 12.0 * s.n);
      hipLaunchKernelGGL(k_group_pack, dim3(grid_for(s.n, B, 8192)), dim3(B), 0, c.s, s, key.p + at, w.p + at);
      DAS_HIP(hipGetLastError());
      at += s.n;
    }
    {
      ProfScope ps(c, "k_group_sort", 4.0 * rows * 3);
      ColSet ks{};
      ks.n = 1;
      ks.c[0] = key.p;
      sort_perm(ks, rows, perm.p, bounded ? bits_for(hi) : 32, c.s);
    }
    uint64_t runs;
    {
      ProfScope ps(c, "k_group_heads", 16.0 * rows + 4.0 * rows);
      runs = scan_total<uint32_t>(HeadIn{key.p, perm.p}, rows, off.p, c.s);
    }
    DBuf<uint64_t> bins(runs, c.s);
    DBuf<uint32_t> run_key(runs, c.s);
    fill_dev(bins.p, 0, 8 * runs, c.s);
    {
      ProfScope ps(c, "k_group_runs", 24.0 * rows + 12.0 * runs);
      hipLaunchKernelGGL(k_group_runs, dim3(grid_for(rows, B, 8192)), dim3(B), 0, c.s, (const uint32_t*)key.p,
                         (const uint64_t*)w.p, (const uint32_t*)perm.p, (const uint32_t*)off.p, rows, bins.p,
                         run_key.p);
      DAS_HIP(hipGetLastError());
    }
    total = compact_bins(c, bins.p, run_key.p, 0, runs);
  } else {
    DBuf<uint64_t> bins(range, c.s);
    fill_dev(bins.p, 0, 8 * range, c.s);
    const bool lds = range <= kGroupLdsBins;
    for (const GroupSrc& s : src) {
      // LDS bins: each workgroup flushes up to `range` adds, so it takes at
      // least kGroupLdsRows rows
      const unsigned grid = lds ? (unsigned)std::min<uint64_t>(std::max<uint64_t>(s.n / kGroupLdsRows, 1), 2048)
                                : grid_for(s.n, B, 8192);
      ProfScope ps(c, lds ? "k_group_accum<true>" : "k_group_accum<false>", src_bytes(s));
      if (lds)
        hipLaunchKernelGGL(k_group_accum<true>, dim3(grid), dim3(B), 0, c.s, s, lo, (uint32_t)range, bins.p, oob.p);
      else
        hipLaunchKernelGGL(k_group_accum<false>, dim3(grid), dim3(B), 0, c.s, s, lo, (uint32_t)range, bins.p, oob.p);
      DAS_HIP(hipGetLastError());
    }
    total = compact_bins(c, bins.p, nullptr, lo, range);
    DAS_CHECK(read_u32(oob.p, c.s) == 0, DAS_E_INVALID, "group counts: a value outside its column's bounds");
  }
  c.group.n = total;
  return total;
}

}  // namespace das
