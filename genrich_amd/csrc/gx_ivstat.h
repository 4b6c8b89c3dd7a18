// gx_ivstat.h -- lengths and per-chromosome tallies of each kept sample's intervals (gx_interval_stats; no Genrich counterpart:
// what deepTools' bamPEFragmentSize or Picard's CollectInsertSizeMetrics and `samtools idxstats` take from another reading of
// the BAM).  (a part of gx_api.hip's translation unit)
//
// A sample's intervals are gx_kept.h's (kept_interval).  One that ends (after clamping) before it starts is INVERTED and has no
// length; every other has L = e - s >= 0 and the weight w = 120 / count.  Wanted, all exact integers:
//   n[L], w120[L]            the intervals of length L and their summed weight
//   nInv, wInv               the inverted ones
//   cn[c], cw120[c]          the intervals on chromosome c (inverted ones included) and their weight
//   cbases120[c]             sum of w L over the intervals on c that have a length
//
// k_ivstat is ONE pass of kept_walk (CNT_NT lanes, CNT_ITEMS events in flight per lane); all of it happens in the walk's stage,
// where every lane of a wavefront is active, so the ballots below see 64 lanes.
//   lengths below IVS_BOUND: two int32 LDS counters per length (a workgroup sees at most CNT_WG_CHUNKS chunks: 120 * events
//     < 2^31, as for kept_window_*), flushed with one 64-bit global add per non-empty counter;
//   the other lengths: (L, n, w) appended to a list, one global counter add per wavefront and step.  When the list is full the
//     kernel keeps counting the entries it would have written and raises IVS_ST_LIST_FULL: the host runs the sample once more
//     with a list of the counted size.  The host sorts and merges the list.
//   When all intervals of a wavefront's step have the same (L, w) -- -j, -y with a fixed extension -- one lane adds popcount
//   times that, once; else every lane adds for itself.
//   chromosomes: the walk gives an interval's chromosome as its first position in tile space; IvsBase[nBase], ascending, names
//     the chromosome (a bounded binary search).  While the intervals of a wavefront's steps lie on ONE chromosome -- nearly
//     always: a coordinate-sorted library, and a name-sorted one whose wavefront happens to -- its lanes add in registers, and
//     the wavefront's sum reaches the counters once, when the chromosome changes or the walk ends.  A step that holds several
//     chromosomes adds per lane.  The counters are 64-bit (w L does not fit 32): an LDS window for chromosomes below
//     IVS_CHROM_WINDOW, global atomics beyond it.
// Every add is an integer's: no result depends on the geometry, the list's capacity or the order of the races.  No workgroup
// waits for another; every loop is bounded.
#pragma once
#include "gx_kept.h"

namespace gx {

constexpr u32 IVS_BOUND = 4096;            // lengths below it are counted in LDS (2 * 16 KiB), the others listed
constexpr u32 IVS_CHROM_WINDOW = 512;      // chromosomes below it are tallied in LDS (3 * 4 KiB)
constexpr u32 IVS_GRID = 512;              // most workgroups unless the chunks or the caller say so: two per CU
constexpr u32 IVS_MAX_GRID = 65535;        // ... and the most a caller may force
constexpr u32 IVS_LIST_CAP = 1u << 16;     // entries of the list at first

// the control words (u64), in front of n[IVS_BOUND], w120[IVS_BOUND], cn[nChrom], cw120[nChrom], cbases120[nChrom]
enum { IVC_NBIG = 0, IVC_STATUS = 1, IVC_NINV = 2, IVC_WINV = 3, IVC_WORDS = 4 };
enum { IVS_ST_LIST_FULL = 1 };

struct IvsBig { u32 len, n; unsigned long long w; };      // n intervals of one length, their weight
struct IvsBase { u64 base; u32 chrom, pad; };             // a chromosome the sample's pileup took, by its first position

struct IvsArgs {
  const CntChunk* chunks;
  u32 nChunks;
  const CntChrom* chroms;
  u32 nChrom;
  const IvsBase* bases;       // [nBase], ascending in base
  u32 nBase;
  unsigned long long* out;    // [IVC_WORDS + 2 * IVS_BOUND + 3 * nChrom]
  IvsBig* big;                // [bigCap]
  u32 bigCap;
};

// the chromosome whose first position is `base` (one of bases[0 .. n), n >= 1)
__device__ __forceinline__ u32 ivs_chrom_of(const IvsBase* __restrict__ bases, u32 n, u64 base) {
  u32 lo = 0, hi = n;
  for (int it = 0; it < 32 && lo + 1 < hi; it++) {
    const u32 mid = (lo + hi) >> 1;
    if (bases[mid].base <= base) lo = mid;
    else hi = mid;
  }
  return bases[lo].chrom;
}

__global__ __launch_bounds__(CNT_NT) void k_ivstat(IvsArgs a) {
  __shared__ int ln[IVS_BOUND], lw[IVS_BOUND];
  __shared__ unsigned long long lc[3 * IVS_CHROM_WINDOW];
  __shared__ long long redN[CNT_NT / 64], redW[CNT_NT / 64];
  for (u32 i = threadIdx.x; i < IVS_BOUND; i += CNT_NT) ln[i] = lw[i] = 0;
  for (u32 i = threadIdx.x; i < 3 * IVS_CHROM_WINDOW; i += CNT_NT) lc[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  unsigned long long* gLen = a.out + IVC_WORDS;
  unsigned long long* gChr = gLen + 2 * IVS_BOUND;
  const u32 nChrom = a.nChrom;
  u32 stat = 0;
  long long invN = 0, invW = 0;                 // (per lane; lane 0 of a wavefront holds its ballots' counts)
  // the chromosome the wavefront is on and what its lanes have added there
  u64 curBase = ~0ull;
  u32 curChrom = 0;
  u32 accN = 0, accW = 0;
  unsigned long long accB = 0;
  auto chrom_add = [&](u32 c, unsigned long long n, unsigned long long w, unsigned long long b) {
    if (c < IVS_CHROM_WINDOW) {
      atomicAdd(&lc[3 * c], n);
      atomicAdd(&lc[3 * c + 1], w);
      if (b) atomicAdd(&lc[3 * c + 2], b);
    } else {
      atomicAdd(&gChr[c], n);
      atomicAdd(&gChr[nChrom + c], w);
      if (b) atomicAdd(&gChr[2 * nChrom + c], b);
    }
  };
  auto chrom_flush = [&]() {   // (every lane of the wavefront)
    if (__ballot(accN != 0)) {
      unsigned long long n = accN, w = accW, b = accB;
      for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o);
        w += __shfl_xor(w, o);
        b += __shfl_xor(b, o);
      }
      if (lane == 0) chrom_add(curChrom, n, w, b);
    }
    accN = accW = 0;
    accB = 0;
  };
  kept_walk(
      a.chunks, a.nChunks, a.chroms, a.nChrom,
      [&](const KeptIv(&iv)[CNT_ITEMS]) {
#pragma unroll
        for (int j = 0; j < CNT_ITEMS; j++) {
          const bool live = iv[j].w != 0;
          const unsigned long long mLive = __ballot(live);
          if (!mLive) continue;   // (wave-uniform)
          const bool inv = live && iv[j].e < iv[j].s, ok = live && !inv;
          const u32 L = ok ? (u32)(iv[j].e - iv[j].s) : 0u, w = (u32)iv[j].w;
          const unsigned long long mInv = __ballot(inv), mOk = mLive & ~mInv;
          if (mInv) {
            if (lane == 0) invN += __popcll(mInv);
            if (inv) invW += w;
          }
          // the lengths
          if (mOk) {
            const int first = __ffsll((long long)mOk) - 1;
            const u32 L0 = (u32)__shfl((int)L, first, 64), w0 = (u32)__shfl((int)w, first, 64);
            if (!__ballot(ok && (L != L0 || w != w0))) {   // one (L, w) in the whole step: one lane adds for all
              if (lane == first) {
                const u32 k = (u32)__popcll(mOk);
                if (L0 < IVS_BOUND) {
                  atomicAdd(&ln[L0], (int)k);
                  atomicAdd(&lw[L0], (int)(k * w0));
                } else {
                  const u32 at = (u32)atomicAdd(&a.out[IVC_NBIG], 1ull);
                  if (at < a.bigCap) a.big[at] = IvsBig{L0, k, (unsigned long long)k * w0};
                  else stat |= IVS_ST_LIST_FULL;
                }
              }
            } else {
              if (ok && L < IVS_BOUND) {
                atomicAdd(&ln[L], 1);
                atomicAdd(&lw[L], (int)w);
              }
              const unsigned long long heavy = __ballot(ok && L >= IVS_BOUND);
              if (heavy) {
                u32 at0 = 0;
                if (lane == 0) at0 = (u32)atomicAdd(&a.out[IVC_NBIG], (unsigned long long)__popcll(heavy));
                at0 = (u32)__shfl((int)at0, 0, 64);
                if (ok && L >= IVS_BOUND) {
                  const u32 at = at0 + (u32)__popcll(heavy & ((1ull << lane) - 1));
                  if (at < a.bigCap) a.big[at] = IvsBig{L, 1u, (unsigned long long)w};
                  else stat |= IVS_ST_LIST_FULL;
                }
              }
            }
          }
          // the chromosomes
          const int firstLive = __ffsll((long long)mLive) - 1;
          const u64 base0 = ((u64)(u32)__shfl((int)(iv[j].base >> 32), firstLive, 64) << 32) | (u32)__shfl((int)(u32)iv[j].base, firstLive, 64);
          if (!__ballot(live && iv[j].base != base0)) {
            if (base0 != curBase) {   // (wave-uniform)
              chrom_flush();
              curBase = base0;
              curChrom = ivs_chrom_of(a.bases, a.nBase, base0);
            }
            if (live) {
              accN++;
              accW += w;
              accB += (unsigned long long)w * L;
            }
          } else if (live) {
            chrom_add(ivs_chrom_of(a.bases, a.nBase, iv[j].base), 1ull, (unsigned long long)w, (unsigned long long)w * L);
          }
        }
      },
      [](const KeptIv&, int) {});
  chrom_flush();
  invN = kept_block_sum(invN, redN);
  invW = kept_block_sum(invW, redW);
  if (threadIdx.x == 0 && invN) {
    atomicAdd(&a.out[IVC_NINV], (unsigned long long)invN);
    atomicAdd(&a.out[IVC_WINV], (unsigned long long)invW);
  }
  if (stat) atomicOr(&a.out[IVC_STATUS], (unsigned long long)stat);
  __syncthreads();
  for (u32 i = threadIdx.x; i < IVS_BOUND; i += CNT_NT) {
    if (ln[i]) atomicAdd(&gLen[i], (unsigned long long)ln[i]);
    if (lw[i]) atomicAdd(&gLen[IVS_BOUND + i], (unsigned long long)lw[i]);
  }
  const u32 nWin = nChrom < IVS_CHROM_WINDOW ? nChrom : IVS_CHROM_WINDOW;
  for (u32 i = threadIdx.x; i < 3 * nWin; i += CNT_NT) {
    const unsigned long long v = lc[i];
    if (v) atomicAdd(&gChr[(i % 3) * nChrom + i / 3], v);
  }
}

}  // namespace gx
