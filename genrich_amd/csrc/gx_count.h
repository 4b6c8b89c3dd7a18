// gx_count.h -- each kept sample's intervals counted in the called peaks (gx_count_in_peaks).  Genrich has no counterpart: its
// intervals (saveInterval / printBED, Genrich.c:2516-2590) end in the pileup; here they are counted once more, against the peaks
// gx_find_peaks left, for FRiP and a per-peak count matrix.
// (a part of gx_api.hip's translation unit)
//
// The intervals, the two event forms, the pass over the chunks and the LDS window are gx_kept.h's.  Coordinates are the
// context's tile space (gx_kept.h), so the peaks of all chromosomes form ONE sorted list of disjoint intervals and an interval
// never meets a peak of another chromosome.  Per interval [s, e): k0 = the first peak with end > s, k1 = the first with
// start >= e; it overlaps peaks k0 .. k1-1 (s < pe && ps < e), i.e. some peak iff k0 < k1.  The tile index (k_cnt_index) gives a
// start for both searches, so an interval costs one index load and one peak load unless it reaches past the end of peak k0.
// Counts go into a difference array over peak index (+w at k0, -w at k1) kept in LDS per workgroup (int32: a workgroup sees at
// most CNT_WG_CHUNKS chunks, 120 * CNT_WG_CHUNKS * CNT_CHUNK < 2^31); one global add per (workgroup, non-zero entry); a scan
// (k_cnt_scan) turns the sums into counts.  More peaks than one LDS window holds: one launch per window.  All sums are integers
// (1/120 units): no result depends on the order of the adds.
#pragma once
#include "gx_kept.h"

namespace gx {

struct CntPeak { u64 s, e; };                        // [start, end) in tile space; entry nPk is a sentinel (both ~0)

constexpr u32 CNT_LDS_MAX = 36864;            // counters per window (144 KiB of the CU's 160)

// idx0[t] = first peak with e > t * TILE, idx1[t] = first peak with s >= t * TILE (t = 0 .. nTiles)
__global__ void k_cnt_index(const CntPeak* __restrict__ pk, u32 nPk, u32 nIdx, u32* __restrict__ idx0, u32* __restrict__ idx1) {
  for (u32 t = blockIdx.x * blockDim.x + threadIdx.x; t < nIdx; t += gridDim.x * blockDim.x) {
    const u64 x = (u64)t << TB;
    u32 lo = 0, hi = nPk;
    while (lo < hi) {
      const u32 m = (lo + hi) >> 1;
      if (pk[m].e > x) hi = m; else lo = m + 1;
    }
    idx0[t] = lo;
    lo = 0;
    hi = nPk;
    while (lo < hi) {
      const u32 m = (lo + hi) >> 1;
      if (pk[m].s >= x) hi = m; else lo = m + 1;
    }
    idx1[t] = lo;
  }
}

struct CntArgs {
  const CntChunk* chunks;
  u32 nChunks;
  const CntChrom* chroms;
  u32 nChrom;
  const CntPeak* pk;
  const u32* idx0;
  const u32* idx1;
  u32 w0, wn;               // this launch's window of the difference array: entries [w0, w0 + wn)
  unsigned long long* diff; // [nPk + 1] (int64 two's complement)
  unsigned long long* tot;  // {total, in_peaks}; null: another window's launch adds them
};

__global__ __launch_bounds__(CNT_NT) void k_cnt_count(CntArgs a) {
  extern __shared__ int cntLds[];
  __shared__ long long red[2][CNT_NT / 64];
  kept_window_clear(cntLds, a.wn);
  long long tot = 0, inp = 0;
  kept_walk(a.chunks, a.nChunks, a.chroms, a.nChrom, [&](const KeptIv& v, int) {
    tot += v.w;
    u32 k0 = a.idx0[v.s >> TB];
    CntPeak P = a.pk[k0];
    while (P.e <= v.s) P = a.pk[++k0];   // (the sentinel ends every scan)
    if (P.s >= v.e) return;
    inp += v.w;
    u32 k1 = k0 + 1;
    if (v.e > P.e) {
      k1 = max(k1, a.idx1[v.e >> TB]);
      while (a.pk[k1].s < v.e) k1++;
    }
    if (k0 - a.w0 < a.wn) atomicAdd(&cntLds[k0 - a.w0], v.w);
    if (k1 - a.w0 < a.wn) atomicAdd(&cntLds[k1 - a.w0], -v.w);
  });
  kept_window_flush(cntLds, a.w0, a.wn, a.diff);
  if (!a.tot) return;
  tot = kept_block_sum(tot, red[0]);
  inp = kept_block_sum(inp, red[1]);
  if (threadIdx.x == 0) {
    if (tot) atomicAdd(a.tot, (unsigned long long)tot);
    if (inp) atomicAdd(a.tot + 1, (unsigned long long)inp);
  }
}

// one workgroup per sample: out[s * stride + k] = sum of diff[s * (nPk + 1) + 0 .. k], k < nPk
__global__ __launch_bounds__(CNT_NT) void k_cnt_scan(const long long* __restrict__ diff, u32 nPk, size_t stride, long long* __restrict__ out) {
  __shared__ long long part[CNT_NT];
  const long long* d = diff + (size_t)blockIdx.x * (nPk + 1);
  long long* o = out + (size_t)blockIdx.x * stride;
  const u32 per = (nPk + CNT_NT - 1) / CNT_NT;
  const u32 lo = min(nPk, threadIdx.x * per), hi = min(nPk, lo + per);
  long long sum = 0;
  for (u32 k = lo; k < hi; k++) sum += d[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < CNT_NT; off <<= 1) {   // inclusive scan of the threads' sums
    const long long v = threadIdx.x >= (u32)off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  long long run = part[threadIdx.x] - sum;
  for (u32 k = lo; k < hi; k++) {
    run += d[k];
    o[k] = run;
  }
}

}  // namespace gx
