// gx_rank.h -- the samples' coverage bins turned into doubled mid-ranks (gx_coverage_rank_gram; no Genrich counterpart: what a
// multiBamSummary / plotCorrelation --corMethod spearman pass takes from a second reading of every BAM).
//
// x_s[b] = sample s's sum120 of bin b (gx_coverage.h).  Over the set B of ranked bins (all of them, or those that are not 0 in
// every sample), for a value v of sample s
//     less_s(v) = #{b in B : x_s[b] < v}      equal_s(v) = #{b in B : x_s[b] == v}      rank2_s(v) = 2 less + equal + 1
// and R_s[b] = rank2_s(x_s[b]) for b in B, 0 outside B.  Everything is an integer; the Gram pass (gx_gram.h) over the rows R_s
// gives what Spearman's rho needs.  Two steps run here, with the host between them (gx_host_rank.h):
//
// 1. k_rank_distinct: one row -> its distinct values with their multiplicities, in an open-addressing table in global memory:
//    keys[cap] (64-bit, RK_EMPTY = free) and counts[cap] (32-bit: a context has at most 2^30 bins).  A slot is claimed with a
//    64-bit compare-and-swap on its key and counted with an atomic add.  A bin track repeats a few thousand values millions of
//    times, so a workgroup keeps a cache of RK_CACHE (value, count) pairs in LDS in front of the table -- the same claim, at most
//    RK_CACHE_PROBES slots tried -- and adds its cache to the table once, at its end; a value that finds no place in the cache
//    goes to the table at once.  Zeros touch neither: a step costs one ballot and one popcount per value slot, added to ctl's
//    zero counter once per wavefront.  Loads are 16 bytes a lane (the rows are 16-byte aligned), two steps loaded before the
//    first is used, as in k_fp_hist.  The table starts small: a claim that brings the used slots above `limit` sets ctl's
//    overflow word, after which every insert returns at once; the host then enlarges the table and runs the row again.
//    k_rank_compact writes the non-empty slots side by side (one atomic per wavefront).  That order is the races'; the host
//    sorts the pairs by value before anybody sees them.
// 2. k_rank: every bin of every sample -> R_s[b], looked up in the sample's table, which the host made from ALL contexts'
//    pairs (gx_rank_tables) and uploaded.  Two forms of the table and of the lookup (Knobs::rankLookup; DESIGN section 4,
//    "Rank correlation of the samples' bins", has the two timings):
//      k_rank<false>  (value ascending, rank2) in two arrays, binary search: log2 D dependent 8-byte loads;
//      k_rank<true>   an open-addressing table of (value, rank2) pairs of 16 bytes, at most half full, hashed by the host with
//                     rk_hash and probed linearly: one 16-byte load gives the key and its rank, 1.5 loads a hit on average.
//    A lane walks the S samples of its bin: once for "is any of them non-zero" (the bins that are 0 everywhere are counted, and
//    with `skip` written as 0 in every row), once for the lookups.  A value that is not in its table sets ctl's missing word.
// k_rank_nzero counts the bins that are 0 in every row and nothing else (the tables need that number before they can be made).
#pragma once
#include "gx_coverage.h"

namespace gx {

constexpr unsigned long long RK_EMPTY = ~0ull;   // (a bin's value is below 2^63)
constexpr int RK_NW = 4;                         // wavefronts per workgroup
constexpr u32 RK_CACHE = 2048;                   // a workgroup's (value, count) pairs in LDS: 24 KiB, six workgroups per CU
constexpr u32 RK_CACHE_PROBES = 4;               // slots tried in the cache before a value goes to the table
constexpr u32 RK_GRID = 1024;                    // most workgroups of a launch unless the caller says so: four per CU
constexpr u32 RK_MAX_GRID = 65535;               // ... and the most a caller may force
constexpr u32 RK_MAX_S = 32;                     // most samples
constexpr int RK_CAP_LOG = 17;                   // log2 of the table's first capacity (Knobs::rankCapLog)
constexpr int RK_CAP_LOG_MAX = 31;               // ... and of its last: 2^30 distinct values at the load limit
constexpr int RK_GROW_LOG = 2;                   // a table that overflowed is made four times as large
// the load limit: cap / 2 used slots.  (gx_rank_geometry reports RK_NW * 64, RK_GRID, RK_CACHE, the first capacity and
// the limit's divisor: the tests take the edges they probe from it)
constexpr u32 RK_LOAD_DIV = 2;
constexpr int RK_LOOKUP = 2;                     // k_rank's lookup unless Knobs::rankLookup says so: 1 binary search, 2 probing
constexpr u32 RK_OVER_EVERY = 16;                // probes of the table between two looks at its overflow word

enum { RKC_ZEROS = 0 /* u64 */, RKC_USED = 2, RKC_OVER = 3, RKC_NOUT = 4, RKC_MISSING = 5, RKC_NZERO = 6 /* u64 */, RKC_WORDS = 8 };

struct RankTab {
  unsigned long long* keys;   // [mask + 1]
  u32* counts;                // [mask + 1]
  u32 mask, limit;
  u32* ctl;                   // [RKC_WORDS]
};

__host__ __device__ __forceinline__ u32 rk_hash(unsigned long long v) {
  v *= 0x9E3779B97F4A7C15ull;
  return (u32)(v >> 32) ^ (u32)(v >> 13);
}

// c more of value v into the table
__device__ __forceinline__ void rk_insert(const RankTab& T, unsigned long long v, u32 c) {
  if (__hip_atomic_load(&T.ctl[RKC_OVER], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // (the row is run again)
  u32 h = rk_hash(v) & T.mask;
  for (u32 probe = 0; probe <= T.mask; probe++, h = (h + 1) & T.mask) {
    // (a full table: no lane walks all of it once another has said so)
    if ((probe & (RK_OVER_EVERY - 1)) == RK_OVER_EVERY - 1 && __hip_atomic_load(&T.ctl[RKC_OVER], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return;
    unsigned long long k = __hip_atomic_load(&T.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == RK_EMPTY) {
      k = atomicCAS(&T.keys[h], RK_EMPTY, v);
      if (k == RK_EMPTY) {
        k = v;
        if (atomicAdd(&T.ctl[RKC_USED], 1u) >= T.limit) atomicOr(&T.ctl[RKC_OVER], 1u);
      }
    }
    if (k == v) {
      atomicAdd(&T.counts[h], c);
      return;
    }
  }
  atomicOr(&T.ctl[RKC_OVER], 1u);   // (every slot holds another value)
}

// one value slot of a wavefront's step: `have` = this lane holds a value of the row
__device__ __forceinline__ void rk_add(unsigned long long v, bool have, u32& zeros, unsigned long long* ck, u32* cc, const RankTab& T) {
  zeros += (u32)__popcll(__ballot(have && v == 0));
  if (!have || v == 0) return;
  u32 h = rk_hash(v) & (RK_CACHE - 1);
  for (u32 probe = 0; probe < RK_CACHE_PROBES; probe++, h = (h + 1) & (RK_CACHE - 1)) {
    unsigned long long k = ck[h];
    if (k == RK_EMPTY) k = atomicCAS(&ck[h], RK_EMPTY, v);
    if (k == RK_EMPTY || k == v) {
      atomicAdd(&cc[h], 1u);
      return;
    }
  }
  rk_insert(T, v, 1u);
}

__global__ __launch_bounds__(RK_NW * 64) void k_rank_distinct(const unsigned long long* __restrict__ row, u64 n, RankTab T) {
  __shared__ unsigned long long ck[RK_CACHE];
  __shared__ u32 cc[RK_CACHE];
  for (u32 k = threadIdx.x; k < RK_CACHE; k += RK_NW * 64) {
    ck[k] = RK_EMPTY;
    cc[k] = 0;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = lane_id();
  const ulonglong2* row2 = reinterpret_cast<const ulonglong2*>(row);
  const u64 n2 = n >> 1;                                              // pairs of values
  const u64 stride = (u64)gridDim.x * (RK_NW * 64);
  u32 zeros = 0;
  for (u64 base = ((u64)blockIdx.x * RK_NW + wv) * 64; base < n2; base += 2 * stride) {   // (wave-uniform: the ballots see 64 lanes)
    const u64 p0 = base + lane, p1 = p0 + stride;
    const bool h0 = p0 < n2, h1 = p1 < n2;
    ulonglong2 a = make_ulonglong2(0, 0), b = make_ulonglong2(0, 0);
    if (h0) a = row2[p0];
    if (h1) b = row2[p1];
    rk_add(a.x, h0, zeros, ck, cc, T);
    rk_add(a.y, h0, zeros, ck, cc, T);
    rk_add(b.x, h1, zeros, ck, cc, T);
    rk_add(b.y, h1, zeros, ck, cc, T);
  }
  if ((n & 1) && blockIdx.x == 0 && wv == 0)                          // the last value of a row of odd length
    rk_add(lane == 0 ? row[n - 1] : 0ull, lane == 0, zeros, ck, cc, T);
  if (lane == 0 && zeros) atomicAdd(reinterpret_cast<unsigned long long*>(T.ctl + RKC_ZEROS), (unsigned long long)zeros);
  __syncthreads();
  for (u32 k = threadIdx.x; k < RK_CACHE; k += RK_NW * 64)
    if (ck[k] != RK_EMPTY) rk_insert(T, ck[k], cc[k]);
}

// the table's non-empty slots side by side: value[i], count[i], i < ctl[RKC_NOUT] afterwards (in no particular order)
__global__ __launch_bounds__(256) void k_rank_compact(RankTab T, unsigned long long* __restrict__ value, unsigned long long* __restrict__ count) {
  const int lane = lane_id();
  const u64 cap = (u64)T.mask + 1;
  for (u64 base = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < cap; base += (u64)gridDim.x * 256) {   // (wave-uniform)
    const u64 h = base + lane;
    const unsigned long long k = h < cap ? T.keys[h] : RK_EMPTY;
    const unsigned long long live = __ballot(k != RK_EMPTY);
    if (!live) continue;
    u32 first = 0;
    if (lane == 0) first = atomicAdd(&T.ctl[RKC_NOUT], (u32)__popcll(live));
    first = (u32)__shfl((int)first, 0, 64);
    if (k != RK_EMPTY) {
      const u32 i = first + (u32)__popcll(live & ((1ull << lane) - 1));
      value[i] = k;
      count[i] = T.counts[h];
    }
  }
}

// ctl[RKC_NZERO] += the bins that are 0 in every one of the S rows
__global__ __launch_bounds__(256) void k_rank_nzero(const unsigned long long* const* __restrict__ rows, u32 S, u64 n, u32* __restrict__ ctl) {
  const int lane = lane_id();
  u32 zeros = 0;
  for (u64 base = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < n; base += (u64)gridDim.x * 256) {   // (wave-uniform)
    const u64 b = base + lane;
    unsigned long long any = 0;
    if (b < n)
      for (u32 s = 0; s < S; s++) any |= rows[s][b];
    zeros += (u32)__popcll(__ballot(b < n && any == 0));
  }
  if (lane == 0 && zeros) atomicAdd(reinterpret_cast<unsigned long long*>(ctl + RKC_NZERO), (unsigned long long)zeros);
}

// sample s's rank2 of v.  Binary search: tabV / tabR [lo, hi), tabV ascending.  Probe: tabV holds (value, rank2) pairs,
// [lo, hi) in pairs, hi - lo a power of two (or 0), RK_EMPTY in a free slot, at most half of the slots used.
template <bool PROBE>
__device__ __forceinline__ unsigned long long rk_lookup(const unsigned long long* __restrict__ tabV, const unsigned long long* __restrict__ tabR,
                                                        u64 lo, u64 hi, unsigned long long v, bool& missing) {
  if constexpr (PROBE) {
    const ulonglong2* pairs = reinterpret_cast<const ulonglong2*>(tabV) + lo;
    const u64 cap = hi - lo;
    u64 h = rk_hash(v) & (cap - 1);
    for (u64 probe = 0; probe < cap; probe++, h = (h + 1) & (cap - 1)) {
      const ulonglong2 e = pairs[h];
      if (e.x == v) return e.y;
      if (e.x == RK_EMPTY) break;
    }
  } else {
    const u64 end = hi;
    while (lo < hi) {   // the first entry that is not below v
      const u64 mid = lo + ((hi - lo) >> 1);
      if (tabV[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end && tabV[lo] == v) return tabR[lo];
  }
  missing = true;
  return 0;
}

// out[s][b] = rank2 of rows[s][b] by sample s's table [off[s], off[s + 1]) of tabV / tabR (rk_lookup); 0 in every row where
// `skip` and the bin is 0 in every row.  ctl[RKC_NZERO] += those bins (with or without `skip`).
template <bool PROBE>
__global__ __launch_bounds__(256) void k_rank(const unsigned long long* const* __restrict__ rows, unsigned long long* const* __restrict__ out, u32 S,
                                              u64 n, const unsigned long long* __restrict__ tabV, const unsigned long long* __restrict__ tabR,
                                              const u64* __restrict__ off, int skip, u32* __restrict__ ctl) {
  const int lane = lane_id();
  u32 zeros = 0;
  bool missing = false;
  for (u64 base = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < n; base += (u64)gridDim.x * 256) {   // (wave-uniform)
    const u64 b = base + lane;
    const bool have = b < n;
    unsigned long long any = 0;
    if (have)
      for (u32 s = 0; s < S; s++) any |= rows[s][b];
    const bool dead = have && any == 0;
    zeros += (u32)__popcll(__ballot(dead));
    if (!have) continue;
    for (u32 s = 0; s < S; s++) {
      unsigned long long r = 0;
      if (!(dead && skip)) r = rk_lookup<PROBE>(tabV, tabR, off[s], off[s + 1], rows[s][b], missing);
      out[s][b] = r;
    }
  }
  if (lane == 0 && zeros) atomicAdd(reinterpret_cast<unsigned long long*>(ctl + RKC_NZERO), (unsigned long long)zeros);
  if (missing) atomicOr(&ctl[RKC_MISSING], 1u);
}

}  // namespace gx
