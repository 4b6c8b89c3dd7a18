// gx_xcor.h -- strand cross-correlation of each sample's 5' ends (gx_set_xcor / gx_push_tags; no Genrich counterpart: the curve
// of phantompeakqualtools / SPP, MACS2 predictd or Q, which otherwise want another tool and another reading of the BAM).
// (a part of gx_api.hip's translation unit)
//
// Two bit vectors per sample over the genome, one per strand, one bit per base, in 64-bit words: base x of a chromosome is bit
// (x & 63) of word off[c] + (x >> 6).  Every chromosome starts on a word boundary, and before and after each one lie `pad` =
// ceil(max(|lo|, |hi|) / 64) + 1 words that stay zero, so that a window shifted by any d in [lo, hi] from a base of a
// chromosome never reads another chromosome's bits and needs no test against the chromosome's ends.  Wanted, exact integers:
//   nP, nM      the set bits of the two vectors
//   n11[d]      the positions x with plus[x] and minus[x + d] on one chromosome, for every d in [lo, hi]
// r(d) = (N n11(d) - nP nM) / sqrt(nP (N - nP) nM (N - nM)) is made of them on the host (gx_emit.cpp).  It uses the UNSHIFTED
// totals: a Pearson coefficient over the windows that overlap at shift d would use the bits of x < len - d only, and differs by
// O(d / len).  This is the definition here, not an approximation of that one.
//
// k_xc_set: one tag per lane, one 64-bit atomicOr.  A tag whose chromosome lies beyond the table, whose position lies at or
//   beyond the chromosome's length, or whose strand is neither 0 nor 1 is counted in a device counter (one add per wavefront)
//   and sets nothing; a tag on a chromosome that takes no part in the sample (skipped, not saved, not owned) sets nothing.
// k_xc_corr: the vectors are cut into tiles of T words (both alike: a word index means the same bases in both).  A workgroup of
//   XC_NT lanes takes tiles blockIdx.x, + gridDim.x, ...  Per tile:
//     the minus words [t T - pad, t T + T + pad] go to LDS (words outside the vector: 0);
//     every wavefront loads 64 plus words per step, coalesced, ballots the non-zero ones and appends them with their word
//       index to a list in LDS (one LDS add per wavefront and step; the order of the list does not matter).  A zero word
//       costs nothing beyond this;
//     then wavefront w takes the blocks of 64 shifts w, w + XC_NW, ...: lane l has the shift s = lo + 64 block + l.  For a
//       plus word P with word index i the 64 minus bits that start at bit 64 i + s are bits o = s & 63 .. of word i + (s >> 6)
//       and, when o != 0, the low bits of the next (never a shift by 64).  P and i are read by all lanes from one LDS address (a
//       broadcast), the lanes' minus words are at most three distinct ones.  The lane adds popcount(P & window) in a register
//       and, after the list, adds the register to its shift's 32-bit LDS counter, which no other lane owns.
//   The LDS counters are 32 bits: a plus word adds at most 64 to a counter, so a workgroup adds them to n11[] (one 64-bit
//   global atomic per shift) and clears them before it has walked more than XC_FLUSH_WORDS = 2^25 plus words (2^25 * 64 = 2^31
//   < 2^32) since the last time, and once at its end.  nP and nM: every lane popcounts the tile words it loads (the tile's own
//   minus words, not the halo), a wavefront sum and one global atomic per wavefront at the end.
//   (Tried and not kept: the list taken 64 entries at a time, one per lane, and handed round by v_readlane, so that only the
//   minus words come from LDS per entry -- 10.3 ms against 9.3 ms on the benchmark's tags, profiles/r21_xcor.txt.)
// Every add is an integer's: the result does not depend on the grid, the tile, the order or the split of the tags.  No
// workgroup waits for another; every loop is bounded.
#pragma once
#include "gx_kernels.h"

namespace gx {

constexpr int XC_MAX_SHIFT = 4096;        // -XC_MAX_SHIFT <= lo <= hi <= XC_MAX_SHIFT
constexpr u32 XC_NT = 256;                // lanes of a workgroup of k_xc_corr (and of k_xc_set)
constexpr u32 XC_NW = XC_NT / 64;
constexpr u32 XC_TILE = 1024;             // plus words per tile unless the caller says so
constexpr u32 XC_MIN_TILE = 64, XC_MAX_TILE = 1024;   // ... a multiple of 64 between these
constexpr u32 XC_GRID = 1024;             // most workgroups unless the caller says so: four per CU
constexpr u32 XC_MAX_GRID = 65535;
constexpr u64 XC_FLUSH_WORDS = 1ull << 25;   // plus words a workgroup walks at most between two flushes of its 32-bit counters
constexpr u64 XC_MAX_BITS = 1ull << 37;   // the genome's bits (with the padding: below 2^32 words)

// the control words (u64) in front of n11[hi - lo + 1]
enum { XCC_NPLUS = 0, XCC_NMINUS = 1, XCC_REJECTED = 2, XCC_WORDS = 4 };

struct XcChrom { u64 off; u32 len, active; };    // first word in the vectors; the bases; takes part in the sample

__host__ __device__ inline u32 xc_pad_words(int lo, int hi) {
  const int m = (lo < 0 ? -lo : lo) > (hi < 0 ? -hi : hi) ? (lo < 0 ? -lo : lo) : (hi < 0 ? -hi : hi);
  return (u32)((m + 63) / 64) + 1;
}
// dynamic LDS of k_xc_corr: the minus span, the list's words, the counters (u32), the list's indices (u32)
__host__ __device__ inline size_t xc_lds_bytes(u32 T, u32 pad, u32 nShift) {
  return ((size_t)T + 2 * pad + 1) * 8 + (size_t)T * 8 + ((size_t)nShift + T) * 4;
}

struct XcTag { u32 chrom, pos, strand; };   // gx_tag

__global__ __launch_bounds__(XC_NT) void k_xc_set(const XcTag* __restrict__ tags, u64 n, const XcChrom* __restrict__ chroms, u32 nChrom,
                                                  unsigned long long* __restrict__ plus, unsigned long long* __restrict__ minus,
                                                  unsigned long long* __restrict__ ctl) {
  const u64 i = (u64)blockIdx.x * XC_NT + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const XcTag t = tags[i];
    if (t.chrom >= nChrom || t.strand > 1u) bad = true;
    else {
      const XcChrom c = chroms[t.chrom];
      if (t.pos >= c.len) bad = true;
      else if (c.active) atomicOr((t.strand ? plus : minus) + c.off + (t.pos >> 6), 1ull << (t.pos & 63u));
    }
  }
  const unsigned long long b = __ballot(bad);
  if (b && (threadIdx.x & 63u) == 0) atomicAdd(ctl + XCC_REJECTED, (unsigned long long)__popcll(b));
}

// nWords: the words of each vector, a multiple of T (the allocation is); the minus words outside [0, nWords) read as 0
__global__ __launch_bounds__(XC_NT) void k_xc_corr(const unsigned long long* __restrict__ plus, const unsigned long long* __restrict__ minus,
                                                   u64 nWords, u32 T, int lo, int hi, unsigned long long* __restrict__ out) {
  extern __shared__ unsigned long long xc_lds[];
  const u32 pad = xc_pad_words(lo, hi);
  const u32 span = T + 2 * pad + 1;
  const u32 nShift = (u32)(hi - lo + 1);
  unsigned long long* lm = xc_lds;              // [span] the minus words from tile start - pad
  unsigned long long* lp = lm + span;           // [T] the tile's non-zero plus words
  u32* acc = reinterpret_cast<u32*>(lp + T);    // [nShift]
  u32* li = acc + nShift;                       // [T] ... and their word index in the tile
  __shared__ u32 nz;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (u32 k = tid; k < nShift; k += XC_NT) acc[k] = 0;
  if (tid == 0) nz = 0;
  __syncthreads();
  const u64 nTiles = nWords / T;
  const u32 nBlocks = (nShift + 63) / 64;
  u64 cntP = 0, cntM = 0, walked = 0;
  for (u64 t = blockIdx.x; t < nTiles; t += gridDim.x) {
    const u64 w0 = t * T;
    if (walked + T > XC_FLUSH_WORDS) {   // (uniform: the counters could wrap with this tile)
      for (u32 k = tid; k < nShift; k += XC_NT) {
        if (acc[k]) atomicAdd(out + XCC_WORDS + k, (unsigned long long)acc[k]);
        acc[k] = 0;
      }
      walked = 0;
      __syncthreads();
    }
    walked += T;
    for (u32 k = tid; k < span; k += XC_NT) {
      const long long g = (long long)w0 - (long long)pad + (long long)k;
      const unsigned long long m = g >= 0 && (u64)g < nWords ? minus[g] : 0ull;
      lm[k] = m;
      if (k >= pad && k < pad + T) cntM += (u64)__popcll(m);
    }
    for (u32 k = tid; k < T; k += XC_NT) {   // (T is a multiple of 64: a wavefront's lanes are all here or all not)
      const unsigned long long p = plus[w0 + k];
      cntP += (u64)__popcll(p);
      const unsigned long long b = __ballot(p != 0);
      u32 base = 0;
      if (lane == 0 && b) base = atomicAdd(&nz, (u32)__popcll(b));
      base = (u32)__shfl((int)base, 0);
      if (p) {
        const u32 at = base + (u32)__popcll(b & ((1ull << lane) - 1ull));
        lp[at] = p;
        li[at] = k;
      }
    }
    __syncthreads();
    const u32 n = nz;
    if (n)
      for (u32 blk = wave; blk < nBlocks; blk += XC_NW) {
        const u32 sh = blk * 64 + lane;
        if (sh < nShift) {
          const int s = lo + (int)sh;
          const int base = (int)pad + (s >> 6);   // (an arithmetic shift: floor) >= 0, and base + i + 1 < span
          const u32 o = (u32)s & 63u;
          u32 c = 0;
          for (u32 j = 0; j < n; j++) {
            const unsigned long long p = lp[j];
            const u32 at = (u32)base + li[j];
            const unsigned long long a = lm[at], b = lm[at + 1];
            const unsigned long long win = o ? (a >> o) | (b << (64u - o)) : a;
            c += (u32)__popcll(p & win);
          }
          acc[sh] += c;
        }
      }
    __syncthreads();
    if (tid == 0) nz = 0;
    __syncthreads();
  }
  for (u32 k = tid; k < nShift; k += XC_NT)
    if (acc[k]) atomicAdd(out + XCC_WORDS + k, (unsigned long long)acc[k]);
  for (int d = 32; d >= 1; d >>= 1) {
    cntP += (u64)__shfl_down((long long)cntP, d);
    cntM += (u64)__shfl_down((long long)cntM, d);
  }
  if (lane == 0) {
    if (cntP) atomicAdd(out + XCC_NPLUS, (unsigned long long)cntP);
    if (cntM) atomicAdd(out + XCC_NMINUS, (unsigned long long)cntM);
  }
}

}  // namespace gx
