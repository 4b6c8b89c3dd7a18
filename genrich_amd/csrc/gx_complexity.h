// gx_complexity.h -- library complexity of each kept sample's intervals (gx_complexity; no Genrich counterpart: what a sorted
// bedpe and an awk line, Picard's EstimateLibraryComplexity or preseq's c_curve take from another reading of the BAM).
// (a part of gx_api.hip's translation unit)
//
// A sample's intervals are gx_kept.h's (kept_interval).  Each is ONE observation of the key (chromosome, start, clamped end);
// wanted are N = observations, D = distinct keys and h[m] = keys seen exactly m times.
//
// The key is 64 bits: (g + 1) << 32 | end, g = the interval's start in tile space (it names the chromosome and the start at
// once), end = its clamped end on the chromosome -- an interval that ends before it starts keeps its end.  The host refuses
// the pass unless the tile space is below 2^32 - 1 bases, so g + 1 fits 32 bits and is never 0: the packing is injective and
// no key equals CPX_EMPTY = 0, which a plain memset makes.
//
// 1. k_cpx_insert: the events -> an open-addressing table of 16-byte slots {key, count, 0} in global memory, a power of two of
//    at least 2 n slots for a sample of n events, sized once (there is no growth path).  A slot is claimed with a 64-bit
//    compare-and-swap on its key and counted with a 32-bit atomic add on the word next to it: key and count share a 16-byte
//    slot, hence a cache line, so an insert touches one line where two arrays would touch two.  Nearly every key of a
//    library is distinct: an LDS cache in front of the table (k_rank_distinct's) would hold singletons only, and there is none.
//    The pass is kept_walk's: CNT_ITEMS events per lane are loaded, then hashed and their home slots read (its stage in
//    between) before the first claim, so that many table lines are in flight per lane.
//    The probe loop is bounded by the capacity, not by the table's sparseness: a key that meets mask + 1 slots of other keys
//    raises CPXC_STATUS (the host: GX_ERR_DEVICE) and is dropped; all lanes then stop early.
// 2. k_cpx_hist: one pass over the slots, 16 bytes a load.  D and h[1] (nearly all keys) are counted by ballot, one add per
//    wavefront and step in a register; multiplicities 2 .. CPX_BOUND - 1 go into a workgroup's LDS histogram, flushed with
//    64-bit global adds for its non-empty classes; a multiplicity of CPX_BOUND or more is appended to a list (one atomic per
//    wavefront and step).  At most n / CPX_BOUND keys can be that frequent, which is the list's capacity; an append beyond it
//    raises CPXC_STATUS too.  The host sorts and run-length encodes the list.
// Every add is an integer's: no result depends on the geometry, the capacity or the order of the races.
#pragma once
#include "gx_kept.h"
#include "gx_rank.h"

namespace gx {

constexpr unsigned long long CPX_EMPTY = 0ull;
constexpr int CPX_NT = CNT_NT;               // lanes of k_cpx_insert's workgroup: kept_walk's
constexpr int CPX_HIST_NT = 256;             // ... and of k_cpx_hist's
constexpr u32 CPX_BOUND = 4096;              // multiplicities below it are counted in LDS (16 KiB), the others listed
constexpr u32 CPX_GRID = 512;                // most workgroups of k_cpx_insert unless the caller says so: two per CU, all its wavefronts
constexpr u32 CPX_HIST_GRID = 2048;          // ... and of k_cpx_hist: eight per CU
constexpr u32 CPX_MAX_GRID = 65535;          // ... and the most a caller may force
constexpr u64 CPX_MAX_SPACE = 0xFFFFFFFFull; // tile space (bases) the key's 32 bits of start hold: g + 1 <= 2^32 - 1
constexpr u32 CPX_OVER_EVERY = 16;           // probes between two looks at the status word

// the control words (u64)
enum { CPXC_N = 0, CPXC_D = 1, CPXC_NBIG = 2, CPXC_STATUS = 3, CPXC_WORDS = 4 };
enum { CPX_ST_TABLE_FULL = 1, CPX_ST_LIST_FULL = 2 };

struct CpxSlot { unsigned long long key; u32 count; u32 pad; };   // 16 bytes, 16-byte aligned

struct CpxTab {
  CpxSlot* slot;              // [mask + 1]
  u32 mask;                   // capacity - 1 (a sample has fewer than 2^31 events: at most 2^32 slots)
  unsigned long long* ctl;    // [CPXC_WORDS]
};

struct CpxArgs {
  const CntChunk* chunks;
  u32 nChunks;
  const CntChrom* chroms;
  u32 nChrom;
  CpxTab T;
};

// one more observation of `key`; k = what its home slot h held when the lane looked (CPX_EMPTY may be stale: the claim decides)
__device__ __forceinline__ void cpx_insert(const CpxTab& T, unsigned long long key, u32 h, unsigned long long k) {
  for (u64 probe = 0;;) {   // (bounded by the capacity: mask + 1 slots are looked at, then the loop gives up)
    if (k == CPX_EMPTY) {
      k = atomicCAS(&T.slot[h].key, CPX_EMPTY, key);
      if (k == CPX_EMPTY) k = key;
    }
    if (k == key) {
      atomicAdd(&T.slot[h].count, 1u);
      return;
    }
    if (++probe > (u64)T.mask) break;
    h = (h + 1) & T.mask;
    // (a table that ran full: no lane walks all of it once another has said so)
    if ((probe & (CPX_OVER_EVERY - 1)) == CPX_OVER_EVERY - 1 &&
        __hip_atomic_load(&T.ctl[CPXC_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return;
    k = __hip_atomic_load(&T.slot[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  atomicOr(&T.ctl[CPXC_STATUS], (unsigned long long)CPX_ST_TABLE_FULL);   // (every slot holds another key)
}

__global__ __launch_bounds__(CPX_NT) void k_cpx_insert(CpxArgs a) {
  __shared__ long long red[CPX_NT / 64];
  long long nObs = 0;
  unsigned long long key[CNT_ITEMS], k0[CNT_ITEMS];
  u32 hs[CNT_ITEMS];
  kept_walk(
      a.chunks, a.nChunks, a.chroms, a.nChrom,
      [&](const KeptIv(&iv)[CNT_ITEMS]) {
#pragma unroll
        for (int j = 0; j < CNT_ITEMS; j++) {
          key[j] = iv[j].w ? ((iv[j].s + 1) << 32) | (iv[j].e - iv[j].base) : CPX_EMPTY;
          hs[j] = iv[j].w ? rk_hash(key[j]) & a.T.mask : 0u;
        }
#pragma unroll
        for (int j = 0; j < CNT_ITEMS; j++)   // the home slots of all of them: CNT_ITEMS table lines in flight per lane
          k0[j] = key[j] == CPX_EMPTY ? CPX_EMPTY : __hip_atomic_load(&a.T.slot[hs[j]].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      },
      [&](const KeptIv&, int j) {
        nObs++;
        cpx_insert(a.T, key[j], hs[j], k0[j]);
      });
  nObs = kept_block_sum(nObs, red);
  if (threadIdx.x == 0 && nObs) atomicAdd(&a.T.ctl[CPXC_N], (unsigned long long)nObs);
}

// hist[m] += the keys seen m times, 1 <= m < CPX_BOUND; big[0 .. ctl[CPXC_NBIG]) = the other keys' multiplicities (in no
// particular order); ctl[CPXC_D] += the keys
__global__ __launch_bounds__(CPX_HIST_NT) void k_cpx_hist(CpxTab T, unsigned long long* __restrict__ hist, u32* __restrict__ big, u32 bigCap) {
  __shared__ u32 lh[CPX_BOUND];
  for (u32 k = threadIdx.x; k < CPX_BOUND; k += CPX_HIST_NT) lh[k] = 0;
  __syncthreads();
  const int lane = lane_id();
  const u64 cap = (u64)T.mask + 1;
  const uint4* slots = reinterpret_cast<const uint4*>(T.slot);
  u32 keys = 0, ones = 0;   // (per wavefront, held by every lane alike: a workgroup's share of the slots is below 2^32)
  for (u64 base = ((u64)blockIdx.x * (CPX_HIST_NT / 64) + (threadIdx.x >> 6)) * 64; base < cap; base += (u64)gridDim.x * CPX_HIST_NT) {   // (wave-uniform)
    const u64 h = base + lane;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (h < cap) v = slots[h];
    const u32 m = (v.x | v.y) ? v.z : 0u;   // (a claimed slot whose count is 0 cannot be: the claim's lane adds to it)
    keys += (u32)__popcll(__ballot(m != 0));
    ones += (u32)__popcll(__ballot(m == 1));
    if (m > 1 && m < CPX_BOUND) atomicAdd(&lh[m], 1u);
    const unsigned long long heavy = __ballot(m >= CPX_BOUND);
    if (heavy) {
      u32 first = 0;
      if (lane == 0) first = (u32)atomicAdd(&T.ctl[CPXC_NBIG], (unsigned long long)__popcll(heavy));
      first = (u32)__shfl((int)first, 0, 64);
      if (m >= CPX_BOUND) {
        const u32 i = first + (u32)__popcll(heavy & ((1ull << lane) - 1));
        if (i < bigCap) big[i] = m;
        else atomicOr(&T.ctl[CPXC_STATUS], (unsigned long long)CPX_ST_LIST_FULL);
      }
    }
  }
  if (lane == 0) {
    if (keys) atomicAdd(&T.ctl[CPXC_D], (unsigned long long)keys);
    if (ones) atomicAdd(&lh[1], ones);
  }
  __syncthreads();
  for (u32 k = threadIdx.x; k < CPX_BOUND; k += CPX_HIST_NT)
    if (lh[k]) atomicAdd(&hist[k], (unsigned long long)lh[k]);
}

}  // namespace gx
