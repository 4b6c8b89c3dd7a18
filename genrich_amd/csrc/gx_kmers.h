// gx_kmers.h -- every k-mer of a set of regions counted on the device (gx_kmer_count_*; no Genrich counterpart: the counting step
// that HOMER, MEME-ChIP or DREME begin with, over the peak sequences cut out of the FASTA once more and a sampled background).
// (a part of gx_api.hip's translation unit)
//
// k is 1 .. KMER_MAX_K.  The window at position x of a region [start, end) of a chromosome is [x, x + k): COUNTED iff
// x + k <= min(end, length) and all k acgt bits are set (k_motif_scan's SCANNED rule with L = k).  Wanted: how often every one of
// the 4^k k-mers is counted, forward strand only, and the counted windows, all exact u64.
//
// k_kmer_count: k_motif_scan's front end (gx_motifs.h: MotRegion records, units of `step` runs of 64 positions, the bounded
//   binary search, the 32-bit windows by funnel shift) with a histogram behind it.  A lane's TABLE INDEX needs no interleaving:
//   ((gc & mask) << k) | (ag & mask), mask = 2^k - 1, is a bijection onto 0 .. 4^k - 1; the host permutes to the public order
//   (A C G T, first base most significant) once when it reads the table back (gx_host_kmers.h: kmer_public).
//   LDS = true (k <= KMER_LDS_MAX_K = 7): the workgroup holds 4^k 32-bit counters (64 KiB at k = 7, two workgroups per CU) and adds
//   with one LDS atomic per counted window.  Non-zero counters go to the 64-bit global table by return-less 64-bit atomics when the
//   workgroup's work ends and before it has walked more than `flushRuns` runs since the last time: its four wavefronts add at
//   most 64 per run to one counter, so with flushRuns <= 2^25 no counter passes 2^31.  (The bound is kept per ROUND of four
//   units: a round that would pass it is preceded by a flush, and a round alone, at most 4 * 16 runs, is always walked.)
//   LDS = false (k = 8 .. 12): return-less 64-bit global atomics straight into the table (128 MiB at k = 12), which the host
//   clears before every pass.
//   Both: when a wavefront's counted lanes all hold one index (homopolymers, simple repeats) one lane adds the popcount
//   (k_ivstat's idiom).  The windows are counted by ballot in lane 0 of each wavefront; one 64-bit add per workgroup at the end.
// Every add is an integer's: no result depends on the launch geometry, the step, the flush bound, the path, the split of the
// pushes or the order of the races.  No workgroup waits for another; every loop is bounded.
#pragma once
#include "gx_motifs.h"

namespace gx {

constexpr u32 KMER_MAX_K = 12;
constexpr u32 KMER_LDS_MAX_K = 7;                // 4^7 counters of 4 bytes: 64 KiB
constexpr u64 KMER_FLUSH_RUNS = MOT_FLUSH_RUNS;  // runs a workgroup walks at most between two flushes of its 32-bit counters

// the control words (u64) next to the table
enum { KMC_WINDOWS = 0, KMC_FLUSHES = 1, KMC_WORDS = 2 };

// the dynamic LDS of a workgroup: the counters (LDS path), and in either path room for the wavefronts' window counts
__host__ __device__ inline size_t kmer_lds_bytes(u32 k, bool lds) {
  const size_t tab = lds ? ((size_t)4 << (2 * k)) : 0, tail = MOT_NW * sizeof(unsigned long long);
  return tab > tail ? tab : tail;
}

struct KmerArgs {
  const unsigned long long *gc, *ag, *acgt;
  const MotRegion* reg;       // [nReg], unit0 ascending, every one with at least one unit
  u32 nReg, nUnits;
  u32 step;                   // runs of 64 positions per unit
  u32 k;
  u64 flushRuns;              // (LDS path) 1 .. KMER_FLUSH_RUNS
  unsigned long long* table;  // [4^k], in table-index order
  unsigned long long* out;    // [KMC_WORDS]
};

template <bool LDS>
__global__ __launch_bounds__(MOT_NT) void k_kmer_count(KmerArgs a) {
  extern __shared__ u32 kmer_lds[];   // LDS: [4^k] counters; at the end, in both paths, MOT_NW u64 window counts
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 k = a.k, mask = (1u << k) - 1u, nTab = 1u << (2u * k);
  if (LDS) {
    for (u32 i = tid; i < nTab; i += MOT_NT) kmer_lds[i] = 0;
    __syncthreads();
  }
  // (workgroup-uniform) the counters to the global table, and cleared
  auto flush = [&]() {
    __syncthreads();
    for (u32 i = tid; i < nTab; i += MOT_NT) {
      const u32 v = kmer_lds[i];
      if (v) {
        atomicAdd(a.table + i, (unsigned long long)v);
        kmer_lds[i] = 0;
      }
    }
    __syncthreads();
  };
  unsigned long long nWin = 0;   // (lane 0) the windows this wavefront counted
  u64 walked = 0;                // runs the workgroup may have walked since its last flush
  const u64 perRound = (u64)MOT_NW * a.step;
  for (u64 u0 = (u64)blockIdx.x * MOT_NW; u0 < a.nUnits; u0 += (u64)gridDim.x * MOT_NW) {
    if (LDS) {   // (u0, walked: workgroup-uniform)
      if (walked && walked + perRound > a.flushRuns) {
        flush();
        if (tid == 0) atomicAdd(a.out + KMC_FLUSHES, 1ull);
        walked = 0;
      }
      walked += perRound;
    }
    const u64 u64u = u0 + wave;
    if (u64u >= a.nUnits) continue;   // (wave-uniform; no barrier below in this iteration)
    const u32 u = (u32)u64u;
    const MotRegion rg = mot_unit_region(a.reg, a.nReg, u);
    for (u32 r = 0; r < a.step; r++) {
      MotLane ln;
      if (!mot_run_lane(a.gc, a.ag, a.acgt, rg, u, a.step, r, lane, ln)) break;   // (wave-uniform)
      const bool ok = ln.room >= k && (ln.wa & mask) == mask;
      const unsigned long long bw = __ballot(ok);
      if (!bw) continue;   // (wave-uniform)
      const u32 idx = ((ln.wg & mask) << k) | (ln.wp & mask);   // < 4^k
      const u32 n = (u32)__popcll(bw);
      if (lane == 0) nWin += n;
      const int first = __ffsll((long long)bw) - 1;
      const u32 idx0 = (u32)__shfl((int)idx, first, 64);
      if (!__ballot(ok && idx != idx0)) {   // one k-mer in the whole run: one lane adds for all
        if ((int)lane == first) {
          if (LDS) atomicAdd(&kmer_lds[idx0], n);
          else atomicAdd(a.table + idx0, (unsigned long long)n);
        }
      } else if (ok) {
        if (LDS) atomicAdd(&kmer_lds[idx], 1u);
        else atomicAdd(a.table + idx, 1ull);
      }
    }
  }
  if (LDS) flush();
  else __syncthreads();
  unsigned long long* wsum = reinterpret_cast<unsigned long long*>(kmer_lds);   // (the counters are flushed: their room is free)
  if (lane == 0) wsum[wave] = nWin;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (u32 w = 0; w < MOT_NW; w++) s += wsum[w];
    if (s) atomicAdd(a.out + KMC_WINDOWS, s);
  }
}

}  // namespace gx
