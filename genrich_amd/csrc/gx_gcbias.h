// gx_gcbias.h -- the reference sequence on the device, GC bias per kept sample and GC content per interval (gx_set_genome /
// gx_push_sequence / gx_gc_bias / gx_gc_content; no Genrich counterpart: deepTools' computeGCBias, the fragment model of
// Benjamini & Speed, which otherwise wants another tool and another reading of the BAM and the genome).
// (a part of gx_api.hip's translation unit)
//
// Two bit vectors over the genome, one bit per base, in 64-bit words: base x of chromosome c is bit (x & 63) of word
// off[c] + (x >> 6).  gc has the bit set for G C g c, acgt for A C G T a c g t; everything else -- N, IUPAC codes, a base never
// pushed, the bits past a chromosome's end, the padding -- is UNKNOWN: both bits 0.  Every chromosome starts on a block of
// GC_BLOCK_WORDS words (512 bases), and before and after each lie at least GC_PAD = GC_MAX_WINDOW / 64 + 1 words that stay zero:
// a window of up to GC_MAX_WINDOW bases that starts on a base of a chromosome never sees a neighbour's bits and needs no test
// against the chromosome's ends.
//
// The window at position x is [x, x + W).  It is CLASSED iff all W of its acgt bits are set, and its class is then g = its gc
// bits, 0 <= g <= W.  Wanted, all exact integers:
//   F[g]            the classed windows that start on a base of a chromosome that takes part      (k_gc_expected)
//   Nn[g], Nw[g]    a sample's intervals whose START's window is classed g, and their weight       (k_gc_observed)
//   nUn, wUn        ... whose window is not classed
//   gc, acgt        the set bits of both vectors inside a given interval                           (k_gc_content)
//
// k_gc_pack: plain sequence bytes to the two vectors.  A lane loads 16 bytes and makes its two 16-bit masks, four lanes join
//   theirs by two shuffles, one of them stores the two words.  A push starts on a word (first_base % 64 == 0), so every word has
//   ONE writer and plain stores suffice; the bytes past the push's end in its last word are unknown (only a chromosome's last
//   push ends inside a word).  The same stretch pushed twice stores the same words twice.
// The rank directory: for each block of 512 bases one 8-byte entry, the gc and the acgt bits before it in its chromosome (two
//   u32).  k_gc_dir_count: a lane per block counts its eight words of each vector.  k_gc_dir_scan: a workgroup per chromosome
//   scans the chromosome's entries in place, GC_DIR_NT at a time, carrying the sum -- nobody waits for anybody.  gc_rank(x) is
//   one entry plus at most eight popcounts per vector.
// k_gc_expected: the streaming pass.  The chromosomes that take part are a list of spans; the tiles of T words of all spans are
//   numbered through, a workgroup takes tiles blockIdx.x, + gridDim.x, ... and finds a tile's span by a bounded binary search.
//   The tile's words of both vectors and the (W >> 6) + 2 words behind them go to LDS.  A lane owns the 64 positions of one
//   word per step: the two counts of its first window from popcounts, then it slides, cnt(x + 1) = cnt(x) - bit(x) + bit(x + W)
//   -- the outgoing bits are its own word, the incoming ones one funnel-shifted pair.  Consecutive windows mostly share g or
//   move by one: the lane carries (g, run length) in registers and adds to the (W + 1) 32-bit LDS counters when g changes.
//   A tile adds at most 64 T to a counter: the workgroup adds the non-empty counters to F (one 64-bit global atomic each)
//   and clears them before it has walked more than `flushWords` <= GC_FLUSH_WORDS = 2^25 words since (2^25 * 64 = 2^31 < 2^32),
//   and once at its end.  The unclassed windows of the words walked are a counter of their own: with the classed ones they must
//   add up to 64 times the words walked, which the host checks.
// k_gc_observed: ONE kept_walk (gx_kept.h) per sample.  The walk gives a chromosome as its first position in tile space;
//   IvsBase (gx_ivstat.h, ivs_chrom_of) names it.  All of a lane's CNT_ITEMS intervals are looked up in the walk's stage --
//   four ranks each, start and start + W (clamped to the length: the bits beyond are zero) in both vectors -- so that their
//   loads are in flight together; the body adds to two (W + 1) int32 LDS windows (kept_window_*: a workgroup sees at most
//   CNT_WG_CHUNKS chunks, 120 * events < 2^31).
// k_gc_content: a lane per interval (chrom, start, end): end clamped to the length, end <= start gives 0; two rank differences.
// Every add is an integer's: no result depends on the launch geometry, the tile, the flush bound, the split of the pushes or
// the order of the races.  No workgroup waits for another; every loop is bounded.
#pragma once
#include "gx_ivstat.h"

namespace gx {

constexpr u32 GC_MAX_WINDOW = 4096;
constexpr u32 GC_PAD = GC_MAX_WINDOW / 64 + 1;   // zero words before and after each chromosome, at least
constexpr u32 GC_BLOCK_WORDS = 8;                // a directory block: 512 bases
constexpr u32 GC_NT = 256;                       // lanes of a workgroup of k_gc_pack, k_gc_dir_count, k_gc_expected, k_gc_content
constexpr u32 GC_DIR_NT = 1024;                  // ... of k_gc_dir_scan
constexpr u32 GC_TILE = 256;                     // words per tile of k_gc_expected unless the caller says so
constexpr u32 GC_MIN_TILE = 64, GC_MAX_TILE = 1024;   // ... a multiple of 64 between these
constexpr u32 GC_GRID = 2048;                    // most workgroups of k_gc_expected unless the caller says so: eight per CU
constexpr u32 GC_OBS_GRID = 512;                 // ... of k_gc_observed: two per CU
constexpr u32 GC_MAX_GRID = 65535;
constexpr u64 GC_FLUSH_WORDS = 1ull << 25;       // words a workgroup walks at most between two flushes of its 32-bit counters
constexpr u64 GC_MAX_BITS = 1ull << 37;          // the genome's bits (with the padding: below 2^32 words)

struct GcChrom { u64 off; u32 len, laid; };      // first word in the vectors (a multiple of GC_BLOCK_WORDS); the bases; has words at all
struct GcSpan { u64 off; u32 words, tile0; };    // a chromosome that takes part: its first word, its words, the tiles before it

// the control words (u64) of k_gc_expected, in front of F[W + 1]; of k_gc_observed, in front of Nn[W + 1], Nw[W + 1]
enum { GCE_UNCLASSED = 0, GCE_WORDS = 2 };
enum { GCO_NUN = 0, GCO_WUN = 1, GCO_WORDS = 2 };

// dynamic LDS of k_gc_expected: both vectors' span, the counters
__host__ __device__ inline u32 gc_span_words(u32 T, u32 W) { return T + (W >> 6) + 2; }
__host__ __device__ inline size_t gc_exp_lds_bytes(u32 T, u32 W) { return (size_t)gc_span_words(T, W) * 16 + ((size_t)W + 1) * 4; }

// a byte's two bits: bit 0 gc, bit 1 acgt
__device__ __forceinline__ u32 gc_class_byte(u32 b) {
  b |= 0x20u;
  const u32 g = (b == 'g' || b == 'c') ? 1u : 0u;
  return g | ((g || b == 'a' || b == 't') ? 2u : 0u);
}

// seq: n bytes from a 16-byte boundary on (the buffer holds whole 16-byte groups); w0: the first word they go to
__global__ __launch_bounds__(GC_NT) void k_gc_pack(const uint4* __restrict__ seq, u64 n, u64 w0, unsigned long long* __restrict__ gc,
                                                   unsigned long long* __restrict__ acgt) {
  const u64 i = (u64)blockIdx.x * GC_NT + threadIdx.x;   // the lane's 16-byte group
  const u64 nGroups = ((n + 63) / 64) * 4;
  u32 mg = 0, ma = 0;
  if (i * 16 < n) {
    const uint4 v = seq[i];
    const u32 d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const u32 c = i * 16 + (u64)k < n ? gc_class_byte((d[k >> 2] >> ((k & 3) * 8)) & 0xffu) : 0u;
      mg |= (c & 1u) << k;
      ma |= (c >> 1) << k;
    }
  }
  const u32 sh = (threadIdx.x & 3u) * 16u;
  unsigned long long g = (unsigned long long)mg << sh, a = (unsigned long long)ma << sh;
  g |= (unsigned long long)__shfl_xor((long long)g, 1);
  a |= (unsigned long long)__shfl_xor((long long)a, 1);
  g |= (unsigned long long)__shfl_xor((long long)g, 2);
  a |= (unsigned long long)__shfl_xor((long long)a, 2);
  if ((threadIdx.x & 3u) == 0 && i < nGroups) {
    gc[w0 + (i >> 2)] = g;
    acgt[w0 + (i >> 2)] = a;
  }
}

// dir[b] = the set bits of block b's eight words, in both vectors (every block of the vectors, the padding's too: zero)
__global__ __launch_bounds__(GC_NT) void k_gc_dir_count(const unsigned long long* __restrict__ gc, const unsigned long long* __restrict__ acgt,
                                                        u64 nBlocks, uint2* __restrict__ dir) {
  const u64 b = (u64)blockIdx.x * GC_NT + threadIdx.x;
  if (b >= nBlocks) return;
  const ulonglong2* pg = reinterpret_cast<const ulonglong2*>(gc + b * GC_BLOCK_WORDS);
  const ulonglong2* pa = reinterpret_cast<const ulonglong2*>(acgt + b * GC_BLOCK_WORDS);
  u32 cg = 0, ca = 0;
#pragma unroll
  for (u32 k = 0; k < GC_BLOCK_WORDS / 2; k++) {
    const ulonglong2 g = pg[k], a = pa[k];
    cg += (u32)__popcll(g.x) + (u32)__popcll(g.y);
    ca += (u32)__popcll(a.x) + (u32)__popcll(a.y);
  }
  dir[b] = make_uint2(cg, ca);
}

// in place, per chromosome: entry k of (len >> 9) + 1 becomes the counts before block k (the last one serves rank(len))
__global__ __launch_bounds__(GC_DIR_NT) void k_gc_dir_scan(const GcChrom* __restrict__ tab, u32 nChrom, uint2* __restrict__ dir) {
  __shared__ u32 shG[GC_DIR_NT / 64], shA[GC_DIR_NT / 64];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (u32 c = blockIdx.x; c < nChrom; c += gridDim.x) {
    const GcChrom cc = tab[c];
    if (!cc.laid) continue;   // (uniform)
    uint2* d = dir + (cc.off / GC_BLOCK_WORDS);
    const u32 nEnt = (cc.len >> 9) + 1;
    u32 carryG = 0, carryA = 0;
    for (u32 base = 0; base < nEnt; base += GC_DIR_NT) {
      const u32 k = base + tid;
      const uint2 v = k < nEnt ? d[k] : make_uint2(0u, 0u);
      u32 g = v.x, a = v.y;
      for (u32 o = 1; o < 64; o <<= 1) {
        const u32 tg = (u32)__shfl_up((int)g, o), ta = (u32)__shfl_up((int)a, o);
        if (lane >= o) {
          g += tg;
          a += ta;
        }
      }
      if (lane == 63) {
        shG[wave] = g;
        shA[wave] = a;
      }
      __syncthreads();
      u32 preG = 0, preA = 0, totG = 0, totA = 0;
      for (u32 w = 0; w < GC_DIR_NT / 64; w++) {
        if (w < wave) {
          preG += shG[w];
          preA += shA[w];
        }
        totG += shG[w];
        totA += shA[w];
      }
      if (k < nEnt) d[k] = make_uint2(carryG + preG + g - v.x, carryA + preA + a - v.y);
      carryG += totG;
      carryA += totA;
      __syncthreads();
    }
  }
}

// the gc and the acgt bits of a chromosome (first word off) before its position x <= len
__device__ __forceinline__ uint2 gc_rank(const unsigned long long* __restrict__ gc, const unsigned long long* __restrict__ acgt,
                                         const uint2* __restrict__ dir, u64 off, u32 x) {
  const u64 blk = off / GC_BLOCK_WORDS + (x >> 9);
  uint2 r = dir[blk];
  const unsigned long long* pg = gc + blk * GC_BLOCK_WORDS;
  const unsigned long long* pa = acgt + blk * GC_BLOCK_WORDS;
  const u32 full = (x >> 6) & 7u, rest = x & 63u;
#pragma unroll
  for (u32 k = 0; k < GC_BLOCK_WORDS; k++)
    if (k < full || (k == full && rest)) {
      const unsigned long long m = k < full ? ~0ull : (1ull << rest) - 1ull;
      r.x += (u32)__popcll(pg[k] & m);
      r.y += (u32)__popcll(pa[k] & m);
    }
  return r;
}

struct GcRegion { u32 chrom, start, end; };   // gx_region

__global__ __launch_bounds__(GC_NT) void k_gc_content(const GcRegion* __restrict__ reg, u64 n, const GcChrom* __restrict__ tab, u32 nChrom,
                                                      const unsigned long long* __restrict__ gc, const unsigned long long* __restrict__ acgt,
                                                      const uint2* __restrict__ dir, unsigned long long* __restrict__ outG,
                                                      unsigned long long* __restrict__ outA) {
  const u64 i = (u64)blockIdx.x * GC_NT + threadIdx.x;
  if (i >= n) return;
  const GcRegion r = reg[i];
  unsigned long long g = 0, a = 0;
  if (r.chrom < nChrom) {
    const GcChrom cc = tab[r.chrom];
    const u32 e = r.end > cc.len ? cc.len : r.end;
    if (cc.laid && r.start < e) {
      const uint2 lo = gc_rank(gc, acgt, dir, cc.off, r.start), hi = gc_rank(gc, acgt, dir, cc.off, e);
      g = hi.x - lo.x;
      a = hi.y - lo.y;
    }
  }
  outG[i] = g;
  outA[i] = a;
}

struct GcExpArgs {
  const unsigned long long *gc, *acgt;
  const GcSpan* spans;        // [nSpan], tile0 ascending
  u32 nSpan, nTiles;
  u32 T, W;
  u64 flushWords;             // T <= flushWords <= GC_FLUSH_WORDS
  unsigned long long* out;    // [GCE_WORDS + W + 1]
};

__global__ __launch_bounds__(GC_NT) void k_gc_expected(GcExpArgs a) {
  extern __shared__ unsigned long long gce_lds[];
  const u32 T = a.T, W = a.W, span = gc_span_words(T, W);
  unsigned long long* lg = gce_lds;                   // [span] the gc words from the tile's first on
  unsigned long long* la = lg + span;                 // [span] ... the acgt words
  u32* cnt = reinterpret_cast<u32*>(la + span);       // [W + 1]
  const u32 tid = threadIdx.x, lane = tid & 63u;
  for (u32 k = tid; k <= W; k += GC_NT) cnt[k] = 0;
  __syncthreads();
  const u32 q = W >> 6, o = W & 63u;
  unsigned long long uncl = 0;
  u64 walked = 0;
  for (u32 t = blockIdx.x; t < a.nTiles; t += gridDim.x) {
    u32 lo = 0, hi = a.nSpan;   // the span of tile t (tile0 <= t, the last such)
    for (int it = 0; it < 32 && lo + 1 < hi; it++) {
      const u32 mid = (lo + hi) >> 1;
      if (a.spans[mid].tile0 <= t) lo = mid;
      else hi = mid;
    }
    const GcSpan sp = a.spans[lo];
    const u32 wFirst = (t - sp.tile0) * T;             // the tile's first word in its chromosome
    const u32 nw = sp.words - wFirst < T ? sp.words - wFirst : T;
    const u64 w0 = sp.off + wFirst;
    if (walked + T > a.flushWords) {   // (uniform: the counters could wrap with this tile)
      __syncthreads();   // (the previous tile's adds are in)
      for (u32 k = tid; k <= W; k += GC_NT) {
        if (cnt[k]) atomicAdd(a.out + GCE_WORDS + k, (unsigned long long)cnt[k]);
        cnt[k] = 0;
      }
      walked = 0;
    }
    walked += T;
    __syncthreads();   // (the previous tile's readers are done with the span; the cleared counters are seen)
    for (u32 k = tid; k < span; k += GC_NT) {   // (the vectors are allocated with this much to spare behind the last chromosome)
      lg[k] = a.gc[w0 + k];
      la[k] = a.acgt[w0 + k];
    }
    __syncthreads();
    for (u32 k = tid; k < nw; k += GC_NT) {
      const unsigned long long G = lg[k], A = la[k];
      u32 cg = 0, ca = 0;
      for (u32 j = 0; j < q; j++) {
        cg += (u32)__popcll(lg[k + j]);
        ca += (u32)__popcll(la[k + j]);
      }
      unsigned long long inG = lg[k + q], inA = la[k + q];
      if (o) {
        const unsigned long long m = (1ull << o) - 1ull;
        cg += (u32)__popcll(inG & m);
        ca += (u32)__popcll(inA & m);
        inG = (inG >> o) | (lg[k + q + 1] << (64u - o));
        inA = (inA >> o) | (la[k + q + 1] << (64u - o));
      }
      u32 cur = 0, run = 0, un = 0;
      for (u32 i = 0; i < 64; i++) {
        if (ca == W) {
          if (cg != cur) {
            if (run) atomicAdd(&cnt[cur], run);
            cur = cg;
            run = 0;
          }
          run++;
        } else {
          un++;
        }
        cg += (u32)((inG >> i) & 1ull) - (u32)((G >> i) & 1ull);
        ca += (u32)((inA >> i) & 1ull) - (u32)((A >> i) & 1ull);
      }
      if (run) atomicAdd(&cnt[cur], run);
      uncl += un;
    }
  }
  __syncthreads();
  for (u32 k = tid; k <= W; k += GC_NT)
    if (cnt[k]) atomicAdd(a.out + GCE_WORDS + k, (unsigned long long)cnt[k]);
  for (int d = 32; d >= 1; d >>= 1) uncl += (unsigned long long)__shfl_down((long long)uncl, d);
  if (lane == 0 && uncl) atomicAdd(a.out + GCE_UNCLASSED, uncl);
}

struct GcObsArgs {
  const CntChunk* chunks;
  u32 nChunks;
  const CntChrom* chroms;
  u32 nChrom;
  const IvsBase* bases;       // [nBase], ascending in base
  u32 nBase;
  const GcChrom* tab;         // [nChrom]
  const unsigned long long *gc, *acgt;
  const uint2* dir;
  u32 W;
  unsigned long long* out;    // [GCO_WORDS + 2 * (W + 1)]
};

__global__ __launch_bounds__(CNT_NT) void k_gc_observed(GcObsArgs a) {
  extern __shared__ int gco_lds[];
  __shared__ long long redN[CNT_NT / 64], redW[CNT_NT / 64];
  const u32 W = a.W, wn = W + 1;
  int* ln = gco_lds;       // [W + 1]
  int* lw = ln + wn;       // [W + 1]
  kept_window_clear(gco_lds, 2 * wn);
  long long unN = 0, unW = 0;
  u32 cls[CNT_ITEMS];
  kept_walk(
      a.chunks, a.nChunks, a.chroms, a.nChrom,
      [&](const KeptIv(&iv)[CNT_ITEMS]) {
        GcChrom cc[CNT_ITEMS];
#pragma unroll
        for (int j = 0; j < CNT_ITEMS; j++) {
          cc[j] = GcChrom{0, 0, 0};
          if (iv[j].w) cc[j] = a.tab[ivs_chrom_of(a.bases, a.nBase, iv[j].base)];
        }
#pragma unroll
        for (int j = 0; j < CNT_ITEMS; j++) {
          cls[j] = ~0u;
          if (iv[j].w && cc[j].laid) {
            const u32 s = (u32)(iv[j].s - iv[j].base);   // (below the length: kept_interval)
            const u32 e = cc[j].len - s < W ? cc[j].len : s + W;
            const uint2 lo = gc_rank(a.gc, a.acgt, a.dir, cc[j].off, s), hi = gc_rank(a.gc, a.acgt, a.dir, cc[j].off, e);
            if (hi.y - lo.y == W) cls[j] = hi.x - lo.x;
          }
        }
      },
      [&](const KeptIv& iv, int j) {
        const u32 g = cls[j];
        if (g <= W) {
          atomicAdd(&ln[g], 1);
          atomicAdd(&lw[g], iv.w);
        } else {
          unN++;
          unW += iv.w;
        }
      });
  unN = kept_block_sum(unN, redN);
  unW = kept_block_sum(unW, redW);
  if (threadIdx.x == 0 && unN) {
    atomicAdd(&a.out[GCO_NUN], (unsigned long long)unN);
    atomicAdd(&a.out[GCO_WUN], (unsigned long long)unW);
  }
  kept_window_flush(gco_lds, 0, 2 * wn, a.out + GCO_WORDS);
}

}  // namespace gx
