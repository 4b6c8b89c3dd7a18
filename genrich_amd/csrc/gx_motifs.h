// gx_motifs.h -- the reference sequence itself on the device and known motifs scanned in it (gx_set_genome_bases /
// gx_get_sequence / gx_set_motifs / gx_motif_scan_*; no Genrich counterpart: what HOMER's findMotifsGenome -find, FIMO or MOODS do
// with the peak sequences cut out of the FASTA once more).
// (a part of gx_api.hip's translation unit)
//
// A third bit vector `ag` next to gc and acgt (gx_gcbias.h: same words, same padding, one writer per word): the bit is set for
// A G a g.  With gc it names a known base: A = (gc 0, ag 1), C = (1, 0), G = (1, 1), T = (0, 0); the complement flips ag.  The
// base's RAW CODE is r = 2 gc + ag: T 0, A 1, C 2, G 3.  A base whose acgt bit is 0 is unknown whatever the other two say.
//
// k_seq_pack3: k_gc_pack with the third mask (k_gc_pack itself keeps its code and serves the contexts without bases).
// k_seq_unpack: four bases per lane back to upper-case letters, N for unknown and for everything past the chromosome's end.
//
// k_motif_scan: motif m of width L (1 .. MOT_MAX_WIDTH) has an L x 4 table of int16 scores and a threshold t.  Its window at
//   position x of a region [start, end) of a chromosome is [x, x + L): SCANNED iff x + L <= min(end, length) and all L acgt bits
//   are set; forward score sum_j s[j][base(x + j)], reverse score sum_j s[j][comp(base(x + L - 1 - j))]; a HIT is a scanned
//   window and a strand whose score is >= t.  Wanted per motif: the scanned windows and the hits of each strand (u64), and, with
//   LIST, every hit as a 16-byte record.
//   The host resolves the regions that can hold a window at all to MotRegion records -- first word, start, clamped end, the
//   caller's index, the units before it -- and a UNIT is `step` runs of 64 positions of one region: a wavefront takes a unit,
//   finds its region by a bounded binary search (as k_gc_expected finds a tile's span), and a lane owns one position of each
//   run.  The lane takes the 32 bits of gc, ag and acgt from x on once, by a funnel shift of two adjacent words of each vector
//   (the words behind a chromosome's last are padding: zero, and allocated), and keeps them in registers for all motifs.
//   The motifs go through LDS in batches of `batch`: per motif MOT_TAB_WORDS = 4 * 32 words, word 4 j + r holding BOTH strands'
//   scores of column j for raw code r -- the forward one in the low half, the reverse one, s[L - 1 - j][r ^ 1], in the high
//   half -- so that one loop and one 4-byte read per column serve both strands.  The lanes of a wavefront are in the same
//   column and read one of four neighbouring words: four banks, broadcast, no conflict.
//   Counts: ballots, lane 0 adds the three popcounts to 32-bit LDS counters; the workgroup adds them to the 64-bit global ones
//   when a batch ends.  A workgroup adds at most 64 per run it walks, its four wavefronts to the same counters: the host
//   chooses (or refuses) the grid so that a WORKGROUP walks at most MOT_FLUSH_RUNS = 2^25 runs per batch (mot_need_grid:
//   2^25 / (step * 4) rounds of four units), 2^25 * 64 = 2^31 < 2^32.
//   Hits: both strands' ballots, one add to the list's counter per wavefront, run and motif that has any (k_ivstat's list
//   idiom); the counter counts past the list's end, and the host runs the pass once more with a list of the counted size.
// Every add is an integer's: no result depends on the launch geometry, the step, the batch, the list's capacity, the split of
// the pushes or the order of the races.  No workgroup waits for another; every loop is bounded.
#pragma once
#include "gx_gcbias.h"

namespace gx {

constexpr u32 MOT_MAX_WIDTH = 32;
constexpr u32 MOT_MAX = 4096;
constexpr u32 MOT_NT = 256;                      // lanes of a workgroup of k_motif_scan, k_seq_unpack
constexpr u32 MOT_NW = MOT_NT / 64;              // its wavefronts
constexpr u32 MOT_GRID = 2048;                   // most workgroups unless the caller says so: eight per CU
constexpr u32 MOT_MAX_GRID = 65535;
constexpr u32 MOT_STEP = 4;                      // runs of 64 positions per unit unless the caller says so
constexpr u32 MOT_MAX_STEP = 16;
constexpr u32 MOT_BATCH = 64;                    // motifs per LDS batch unless the caller says so, and at most
constexpr u32 MOT_TAB_WORDS = 4 * MOT_MAX_WIDTH; // words of a motif's table
constexpr u64 MOT_LIST_MIN = 1ull << 16;         // the first list's entries, at least
constexpr u64 MOT_FLUSH_RUNS = 1ull << 25;       // runs a workgroup walks at most per batch (its 32-bit counters)
constexpr u64 MOT_MAX_HITS = 1ull << 31;
constexpr u64 MOT_LIST_SHARE = 2048;              // the first list holds a hit in this many windows of every motif (both strands together)
constexpr u64 MOT_LIST_FIRST_MAX = 1ull << 24;   // ... and at most this many entries (256 MiB), unless the caller says so

// The least grid with which no workgroup walks more than MOT_FLUSH_RUNS runs per batch.  A workgroup's MOT_NW wavefronts take a
// unit of `step` runs each per round and add to the SAME counters: it may walk MOT_FLUSH_RUNS / (step * MOT_NW) rounds.
__host__ __device__ inline u64 mot_need_grid(u64 nUnits, u32 step) {
  const u64 rounds = (nUnits + MOT_NW - 1) / MOT_NW, wgRounds = MOT_FLUSH_RUNS / ((u64)step * MOT_NW);
  return (rounds + wgRounds - 1) / wgRounds;
}

struct MotMeta { u32 width; int thr; };                      // a motif on the device, next to its table
struct MotRegion { u64 off; u32 start, end, region, unit0; };// first word of its chromosome; [start, end) clamped; the caller's index; units before it
struct MotHit { u32 region, pos; int score; uint16_t motif; uint8_t strand, pad; };   // gx_motif_hit

// the control words (u64) in front of the counts [3 * nMotif]: windows, hits +, hits - per motif
enum { MOC_STATUS = 0, MOC_COUNT = 1, MOC_WORDS = 2 };
enum : u64 { MOT_ST_LIST_FULL = 1 };

__host__ __device__ inline size_t mot_lds_bytes(u32 batch) { return (size_t)batch * (MOT_TAB_WORDS * 4 + sizeof(MotMeta) + 3 * 4); }

// a byte's three bits: bit 0 gc, bit 1 acgt, bit 2 ag
__device__ __forceinline__ u32 seq_class_byte(u32 b) {
  b |= 0x20u;
  const u32 g = (b == 'g' || b == 'c') ? 1u : 0u;
  const u32 k = (g || b == 'a' || b == 't') ? 2u : 0u;
  return g | k | ((b == 'a' || b == 'g') ? 4u : 0u);
}

// k_gc_pack's arguments and the third vector
__global__ __launch_bounds__(GC_NT) void k_seq_pack3(const uint4* __restrict__ seq, u64 n, u64 w0, unsigned long long* __restrict__ gc,
                                                     unsigned long long* __restrict__ acgt, unsigned long long* __restrict__ ag) {
  const u64 i = (u64)blockIdx.x * GC_NT + threadIdx.x;   // the lane's 16-byte group
  const u64 nGroups = ((n + 63) / 64) * 4;
  u32 mg = 0, ma = 0, mp = 0;
  if (i * 16 < n) {
    const uint4 v = seq[i];
    const u32 d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const u32 c = i * 16 + (u64)k < n ? seq_class_byte((d[k >> 2] >> ((k & 3) * 8)) & 0xffu) : 0u;
      mg |= (c & 1u) << k;
      ma |= ((c >> 1) & 1u) << k;
      mp |= (c >> 2) << k;
    }
  }
  const u32 sh = (threadIdx.x & 3u) * 16u;
  unsigned long long g = (unsigned long long)mg << sh, a = (unsigned long long)ma << sh, p = (unsigned long long)mp << sh;
  g |= (unsigned long long)__shfl_xor((long long)g, 1);
  a |= (unsigned long long)__shfl_xor((long long)a, 1);
  p |= (unsigned long long)__shfl_xor((long long)p, 1);
  g |= (unsigned long long)__shfl_xor((long long)g, 2);
  a |= (unsigned long long)__shfl_xor((long long)a, 2);
  p |= (unsigned long long)__shfl_xor((long long)p, 2);
  if ((threadIdx.x & 3u) == 0 && i < nGroups) {
    gc[w0 + (i >> 2)] = g;
    acgt[w0 + (i >> 2)] = a;
    ag[w0 + (i >> 2)] = p;
  }
}

// out[4 k .. 4 k + 3] = the bases start + 4 k .. of the chromosome at word `off` (laid: it has words at all); n4 groups
__global__ __launch_bounds__(MOT_NT) void k_seq_unpack(const unsigned long long* __restrict__ gc, const unsigned long long* __restrict__ ag,
                                                       const unsigned long long* __restrict__ acgt, u64 off, u32 len, u32 laid, u64 start, u64 n4,
                                                       u32* __restrict__ out) {
  const u64 k = (u64)blockIdx.x * MOT_NT + threadIdx.x;
  if (k >= n4) return;
  u32 v = 0;
#pragma unroll
  for (u32 j = 0; j < 4; j++) {
    const u64 x = start + 4 * k + j;
    u32 ch = 'N';
    if (laid && x < len) {
      const u64 w = off + (x >> 6);
      const u32 b = (u32)(x & 63u);
      if ((acgt[w] >> b) & 1ull) {
        const u32 r = (u32)((gc[w] >> b) & 1ull) * 2u + (u32)((ag[w] >> b) & 1ull);
        ch = r == 0 ? 'T' : r == 1 ? 'A' : r == 2 ? 'C' : 'G';
      }
    }
    v |= ch << (8 * j);
  }
  out[k] = v;
}

struct MotArgs {
  const unsigned long long *gc, *ag, *acgt;
  const MotRegion* reg;       // [nReg], unit0 ascending, every one with at least one unit
  u32 nReg, nUnits;
  u32 step;                   // runs of 64 positions per unit
  const int* tabs;            // [nMotif][MOT_TAB_WORDS]
  const MotMeta* meta;        // [nMotif]
  u32 nMotif, batch;
  MotHit* list;
  u32 listCap;
  unsigned long long* out;    // [MOC_WORDS + 3 * nMotif]
};

// the 32 bits of a vector from bit `sh` of word w on
__device__ __forceinline__ u32 mot_window(const unsigned long long* __restrict__ v, u64 w, u32 sh) {
  const unsigned long long lo = v[w], hi = v[w + 1];
  return (u32)(sh ? (lo >> sh) | (hi << (64u - sh)) : lo);
}

// The front end k_motif_scan shares with k_kmer_count (gx_kmers.h).
// the region of unit u (unit0 <= u, the last such): a bounded binary search
__device__ __forceinline__ MotRegion mot_unit_region(const MotRegion* __restrict__ reg, u32 nReg, u32 u) {
  u32 lo = 0, hi = nReg;
  for (int it = 0; it < 32 && lo + 1 < hi; it++) {
    const u32 mid = (lo + hi) >> 1;
    if (reg[mid].unit0 <= u) lo = mid;
    else hi = mid;
  }
  return reg[lo];
}
// a lane's position in run k of unit u of its region: x, the bases from x to the region's end (0: none) and the 32 bits of each
// vector from x on; false (wave-uniform) when the run lies behind the region's end
struct MotLane { u64 x; u32 room, wg, wp, wa; };
__device__ __forceinline__ bool mot_run_lane(const unsigned long long* __restrict__ gc, const unsigned long long* __restrict__ ag,
                                             const unsigned long long* __restrict__ acgt, const MotRegion& rg, u32 u, u32 step, u32 k, u32 lane,
                                             MotLane& L) {
  const u64 first = (u64)rg.start + ((u64)(u - rg.unit0) * step + k) * 64u;   // the run's first position
  if (first >= rg.end) return false;
  L.x = first + lane;
  L.room = L.x < rg.end ? (u32)(rg.end - L.x) : 0u;
  L.wg = L.wp = L.wa = 0;
  if (L.room) {
    const u64 w = rg.off + (L.x >> 6);
    const u32 sh = (u32)(L.x & 63u);
    L.wg = mot_window(gc, w, sh);
    L.wp = mot_window(ag, w, sh);
    L.wa = mot_window(acgt, w, sh);
  }
  return true;
}

template <bool LIST>
__global__ __launch_bounds__(MOT_NT) void k_motif_scan(MotArgs a) {
  extern __shared__ int mot_lds[];
  const u32 B = a.batch;
  int* tab = mot_lds;                                                  // [B][MOT_TAB_WORDS]
  MotMeta* meta = reinterpret_cast<MotMeta*>(tab + B * MOT_TAB_WORDS); // [B]
  u32* cnt = reinterpret_cast<u32*>(meta + B);                         // [B][3]
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  u32 stat = 0;
  for (u32 m0 = 0; m0 < a.nMotif; m0 += B) {
    const u32 nb = a.nMotif - m0 < B ? a.nMotif - m0 : B;
    __syncthreads();   // (the previous batch's readers and its flush are done)
    for (u32 k = tid; k < nb * MOT_TAB_WORDS; k += MOT_NT) tab[k] = a.tabs[(size_t)m0 * MOT_TAB_WORDS + k];
    for (u32 k = tid; k < nb; k += MOT_NT) meta[k] = a.meta[m0 + k];
    for (u32 k = tid; k < 3 * nb; k += MOT_NT) cnt[k] = 0;
    __syncthreads();
    for (u64 u0 = (u64)blockIdx.x * MOT_NW; u0 < a.nUnits; u0 += (u64)gridDim.x * MOT_NW) {
      const u64 u64u = u0 + wave;
      if (u64u >= a.nUnits) continue;   // (wave-uniform)
      const u32 u = (u32)u64u;
      const MotRegion rg = mot_unit_region(a.reg, a.nReg, u);
      for (u32 k = 0; k < a.step; k++) {
        MotLane ln;
        if (!mot_run_lane(a.gc, a.ag, a.acgt, rg, u, a.step, k, lane, ln)) break;   // (wave-uniform)
        const u64 x = ln.x;
        const u32 room = ln.room, wg = ln.wg, wp = ln.wp, wa = ln.wa;
        for (u32 m = 0; m < nb; m++) {
          const MotMeta mm = meta[m];
          const u32 L = mm.width, mask = L >= 32u ? ~0u : (1u << L) - 1u;
          const bool ok = room >= L && (wa & mask) == mask;
          const int* t = tab + m * MOT_TAB_WORDS;
          int f = 0, r = 0;
          for (u32 j = 0; j < L; j++) {
            const int v = t[4u * j + ((wg >> j) & 1u) * 2u + ((wp >> j) & 1u)];
            f += (int)(short)(v & 0xffff);
            r += v >> 16;
          }
          const bool hf = ok && f >= mm.thr, hr = ok && r >= mm.thr;
          const unsigned long long bw = __ballot(ok);
          if (!bw) continue;   // (wave-uniform)
          const unsigned long long bf = __ballot(hf), br = __ballot(hr);
          if (lane == 0) {
            atomicAdd(&cnt[3 * m], (u32)__popcll(bw));
            if (bf) atomicAdd(&cnt[3 * m + 1], (u32)__popcll(bf));
            if (br) atomicAdd(&cnt[3 * m + 2], (u32)__popcll(br));
          }
          if (LIST && (bf | br)) {
            const u32 nf = (u32)__popcll(bf);
            unsigned long long at0 = 0;
            if (lane == 0) at0 = atomicAdd(&a.out[MOC_COUNT], (unsigned long long)(nf + (u32)__popcll(br)));
            at0 = ((unsigned long long)(u32)__shfl((int)(at0 >> 32), 0, 64) << 32) | (u32)__shfl((int)(u32)at0, 0, 64);
            const u32 pos = (u32)(x - rg.start);
            if (hf) {
              const unsigned long long at = at0 + (u32)__popcll(bf & below);
              if (at < a.listCap) a.list[at] = MotHit{rg.region, pos, f, (uint16_t)(m0 + m), 0, 0};
              else stat |= (u32)MOT_ST_LIST_FULL;
            }
            if (hr) {
              const unsigned long long at = at0 + nf + (u32)__popcll(br & below);
              if (at < a.listCap) a.list[at] = MotHit{rg.region, pos, r, (uint16_t)(m0 + m), 1, 0};
              else stat |= (u32)MOT_ST_LIST_FULL;
            }
          }
        }
      }
    }
    __syncthreads();
    for (u32 k = tid; k < 3 * nb; k += MOT_NT)
      if (cnt[k]) atomicAdd(a.out + MOC_WORDS + 3 * (size_t)m0 + k, (unsigned long long)cnt[k]);
  }
  if (LIST && stat) atomicOr(a.out + MOC_STATUS, (unsigned long long)stat);
}

}  // namespace gx
