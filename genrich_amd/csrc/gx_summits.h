// gx_summits.h -- the local maxima of the POOLED treatment depth inside each called peak (gx_peak_summits): a narrowPeak line
// has one summit; a wide peak over two binding sites has two maxima, and everything centred on summits wants both.  Genrich has
// no counterpart.
// (a part of gx_api.hip's translation unit)
//
// The definition ("Summits inside peaks"):
//   pooled depth  the sum over the kept TREATMENT samples (controls never) of the depth gx_peak_signal defines (gx_peaksig.h):
//                 +w at s, -w at the clamped e, w = 120 / count; empty intervals add nothing, e < s adds -w over [e, s); -E
//                 regions are not masked.  Per peak [ps, pe): d(x), x in [0, L), int64 in 1/120 units.
//   plateau       a maximal run [a, b) of equal d; a LOCAL MAXIMUM when d is strictly lower on both sides, a side outside the
//                 peak counting as lower.
//   per local maximum of height h:  pos = a + (b - a - 1) / 2, width = b - a, prominence = h - max(baseL, baseR).  A side's
//                 base is the minimum of d over the bases between the plateau and the nearest base on that side with d > h
//                 (strictly), or up to the peak's end when there is none.  A side whose range is empty (the plateau touches
//                 the peak's edge) is left out of the max; both empty (the plateau is the whole peak): the base is 0.
//   reported      the peak's highest local maximum (the leftmost of equals) when h > 0; every other local maximum with h > 0
//                 and  prominence * 100 >= P * h  and  h * 100 >= R * hmax  (integers; equality keeps it).  A peak whose pooled
//                 depth is nowhere positive has none.
//
// The pooled PEAK SPACE is gx_peaksig.h's buffer, cleared once and written by the unchanged k_psig_scatter, sample after sample.
// k_summits gives a wavefront per peak, striding over the peaks as k_psig_reduce does: the same 16-byte loads and 64-bit scan;
// a base starts a RUN when its depth differs from the base before it (the lane before, or the step before: that depth is
// carried), bases behind L start none.  The runs (start, value) are compacted by ballot and popcount into the wavefront's
// buffer: SUM_RUN_CAP runs of LDS each.  A peak with more runs is flagged with its run total and left to a second launch,
// k_summits<true>, whose buffers lie in an HBM scratch of the counted size.  Adjacent runs differ, so run i is a local maximum
// when both neighbours are lower.  A lane per run: the candidates (local maxima that pass the height rule, and the highest)
// walk outwards over the runs for their bases, up to the first higher run.  The runs stand in BLOCKS of SUM_BLK with each
// block's maximum and minimum beside them: a walk goes run by run to the end of its own block, block by block while the
// block's maximum is not higher, and run by run through the block that ends it -- at most 2 SUM_BLK + n / SUM_BLK steps a side
// for a peak of n runs, whatever its shape.  Every loop is bounded by n; a sawtooth of equal teeth, every tooth's walk
// crossing the whole peak, is the worst case: n / 64 rounds of a wavefront of that many steps (tools/summits_bench.py
// measures it).  The reported summits go to one list by ballot, popcount and one counter add per
// wavefront and 64 runs; the counter counts past the list's end (gx_host_kept.h counted_list).  No workgroup waits for another.
// All figures are exact integers: none depends on the grid or on the order of the adds.
#pragma once
#include "gx_peaksig.h"
#include "gx_pileup.h"

namespace gx {

constexpr int SUM_NT = 256;                   // four wavefronts, a peak each
constexpr u32 SUM_GRID = 2048;                // at most so many workgroups, striding over the peaks
constexpr u32 SUM_RUN_CAP = 1024;             // runs of a peak in LDS: 12 bytes each, 12 KiB a wavefront, 48 KiB a workgroup
constexpr u32 SUM_BLK = 64;                   // runs of a block (a lane each when its maximum and minimum are taken)
constexpr u64 SUM_LIST_MIN = 4096;            // the list's first capacity: max(SUM_LIST_MIN, 2 * peaks)

enum { SMC_STATUS = 0, SMC_COUNT = 1, SMC_NFLAG = 2, SMC_FLAGRUNS = 3, SMC_WORDS = 4 };   // the control words (u64)
constexpr unsigned long long SUM_ST_LIST_FULL = 1, SUM_ST_RUNS = 2;   // RUNS: a flagged peak had more runs than counted

struct SumRec { u32 peak, pos, width, pad; long long height, prom; };   // = gx_summit
struct SumBig { u32 peak, runs; u64 off, boff; };                       // a flagged peak: its runs' and its blocks' place in the scratch

struct SumArgs {
  const int* space;
  const u64* off;           // [nPk] first slot of each peak
  const CntPeak* pk;
  u32 nPk;
  u32 P, R;                 // the two percentages
  u32 runCap;               // first launch: runs a wavefront holds (<= SUM_RUN_CAP)
  u32* flag;                // first launch: [nPk], cleared; the run total of a peak with more than runCap
  const SumBig* big;        // second launch: the flagged peaks
  u32 nBig;
  u32* scrStart;            // ... and the scratch their runs go to
  long long* scrVal;
  long long* scrBlk;        // ... and their blocks' {max, min}
  SumRec* list;
  u32 listCap;
  unsigned long long* out;  // [SMC_WORDS]
};

// one peak by one wavefront; rs / rv: room for cap runs, bm: for {max, min} of every SUM_BLK of them (LDS or HBM)
template <bool BIG>
__device__ __forceinline__ void summits_of_peak(const SumArgs& a, u32 k, u32* rs, long long* rv, long long* bm, u32 cap, u32 lane) {
  const CntPeak P = a.pk[k];
  const u64 L = P.e - P.s;
  const int4* row = reinterpret_cast<const int4*>(a.space + a.off[k]);
  const u64 lower = (1ull << lane) - 1ull;
  long long carry = 0, prevLast = 0;
  u32 n = 0;
  for (u64 b = 0; b < L; b += PSIG_STEP) {
    const u64 x0 = b + lane * PSIG_PAD;
    int4 d = make_int4(0, 0, 0, 0);
    if (x0 < L) d = row[x0 >> 2];    // (the padding holds zeros)
    long long v[4];
    v[0] = d.x;
    v[1] = v[0] + d.y;
    v[2] = v[1] + d.z;
    v[3] = v[2] + d.w;
    long long incl = v[3];
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(incl, o);
      if (lane >= (u32)o) incl += t;
    }
    const long long before = carry + incl - v[3];
    carry += __shfl(incl, 63);
    long long prev = __shfl_up(before + v[3], 1);   // the depth of the base before this lane's first
    if (lane == 0) prev = prevLast;
    prevLast = __shfl(before + v[3], 63);           // (read again only after a whole step: a base of the peak)
    bool st[4];
    u64 m[4];
    u32 at = n;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u64 x = x0 + j;
      const long long depth = before + v[j];
      st[j] = x < L && (x == 0 || depth != prev);
      prev = depth;
      m[j] = __ballot(st[j]);
      at += (u32)__popcll(m[j] & lower);
      n += (u32)__popcll(m[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (st[j]) {
        if (at < cap) {
          rs[at] = (u32)(x0 + j);
          rv[at] = before + v[j];
        }
        at++;
      }
  }
  if (n > cap) {
    if (lane == 0) {
      if (BIG) atomicOr(a.out + SMC_STATUS, SUM_ST_RUNS);
      else {
        a.flag[k] = n;
        atomicAdd(a.out + SMC_NFLAG, 1ull);
        atomicAdd(a.out + SMC_FLAGRUNS, (unsigned long long)n);
      }
    }
    return;
  }
  if (BIG) __threadfence();   // (the runs lie in HBM: this wavefront's other lanes read them next)
  pile_sync();
  // the highest run, the leftmost of equals (a local maximum: its neighbours differ from it)
  long long hmax = LLONG_MIN;
  u32 imax = ~0u;
  for (u32 i = lane; i < n; i += 64) {
    const long long h = rv[i];
    if (h > hmax) {
      hmax = h;
      imax = i;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const long long oh = __shfl_xor(hmax, o);
    const u32 oi = __shfl_xor(imax, o);
    if (oh > hmax || (oh == hmax && oi < imax)) {
      hmax = oh;
      imax = oi;
    }
  }
  if (hmax <= 0) return;
  for (u32 b0 = 0; b0 < n; b0 += SUM_BLK) {    // the blocks' maxima and minima
    const u32 i = b0 + lane;
    long long hi = i < n ? rv[i] : LLONG_MIN, lo = i < n ? rv[i] : LLONG_MAX;
    for (int o = 32; o > 0; o >>= 1) {
      hi = max(hi, __shfl_xor(hi, o));
      lo = min(lo, __shfl_xor(lo, o));
    }
    if (lane == 0) {
      bm[2 * (b0 / SUM_BLK)] = hi;
      bm[2 * (b0 / SUM_BLK) + 1] = lo;
    }
  }
  if (BIG) __threadfence();
  pile_sync();
  for (u32 i0 = 0; i0 < n; i0 += 64) {
    const u32 i = i0 + lane;
    bool cand = false;
    long long h = 0, prom = 0;
    if (i < n) {
      h = rv[i];
      cand = h > 0 && (i == 0 || rv[i - 1] < h) && (i + 1 == n || rv[i + 1] < h) && (i == imax || h * 100 >= (long long)a.R * hmax);
    }
    if (cand) {
      long long bl = LLONG_MAX, br = LLONG_MAX;
      {                                // to the left: the runs below i
        u32 j = i;
        bool ended = false;
        for (const u32 stop = i & ~(SUM_BLK - 1); j > stop;) {
          const long long t = rv[--j];
          if (t > h) {
            ended = true;
            break;
          }
          bl = min(bl, t);
        }
        if (!ended) {
          while (j > 0 && bm[2 * (j / SUM_BLK - 1)] <= h) {   // (j is a block's first run)
            bl = min(bl, bm[2 * (j / SUM_BLK - 1) + 1]);
            j -= SUM_BLK;
          }
          for (const u32 stop = j > 0 ? j - SUM_BLK : 0; j > stop;) {
            const long long t = rv[--j];
            if (t > h) break;
            bl = min(bl, t);
          }
        }
      }
      {                                // to the right: the runs above i
        u32 j = i + 1;
        bool ended = false;
        for (const u32 stop = min(n, (i | (SUM_BLK - 1)) + 1); j < stop; j++) {
          const long long t = rv[j];
          if (t > h) {
            ended = true;
            break;
          }
          br = min(br, t);
        }
        if (!ended) {
          while (j < n && bm[2 * (j / SUM_BLK)] <= h) {       // (j is a block's first run)
            br = min(br, bm[2 * (j / SUM_BLK) + 1]);
            j = min(n, j + SUM_BLK);
          }
          for (const u32 stop = min(n, j + SUM_BLK); j < stop; j++) {
            const long long t = rv[j];
            if (t > h) break;
            br = min(br, t);
          }
        }
      }
      const long long base = i == 0 ? (i + 1 == n ? 0 : br) : (i + 1 == n ? bl : max(bl, br));
      prom = h - base;
      cand = i == imax || prom * 100 >= (long long)a.P * h;
    }
    const u64 rep = __ballot(cand);
    if (!rep) continue;              // (wave-uniform)
    unsigned long long first = 0;
    if (lane == 0) first = atomicAdd(a.out + SMC_COUNT, (unsigned long long)__popcll(rep));
    first = __shfl(first, 0);
    const unsigned long long slot = first + (unsigned long long)__popcll(rep & lower);
    if (cand) {
      if (slot < a.listCap) {
        const u32 s0 = rs[i], e0 = i + 1 == n ? (u32)L : rs[i + 1];
        a.list[slot] = SumRec{k, s0 + (e0 - s0 - 1) / 2, e0 - s0, 0u, h, prom};
      } else {
        atomicOr(a.out + SMC_STATUS, SUM_ST_LIST_FULL);
      }
    }
  }
}

template <bool BIG>
__global__ __launch_bounds__(SUM_NT) void k_summits(SumArgs a) {
  __shared__ u32 sStart[BIG ? 1 : (SUM_NT / 64) * SUM_RUN_CAP];
  __shared__ long long sVal[BIG ? 1 : (SUM_NT / 64) * SUM_RUN_CAP];
  __shared__ long long sBlk[BIG ? 1 : (SUM_NT / 64) * 2 * (SUM_RUN_CAP / SUM_BLK)];
  const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, wpb = SUM_NT / 64;
  if (BIG) {
    for (u32 q = blockIdx.x * wpb + wv; q < a.nBig; q += gridDim.x * wpb) {
      const SumBig g = a.big[q];
      summits_of_peak<true>(a, g.peak, a.scrStart + g.off, a.scrVal + g.off, a.scrBlk + g.boff, g.runs, lane);
    }
  } else {
    for (u32 k = blockIdx.x * wpb + wv; k < a.nPk; k += gridDim.x * wpb) {
      summits_of_peak<false>(a, k, sStart + wv * SUM_RUN_CAP, sVal + wv * SUM_RUN_CAP, sBlk + wv * 2 * (SUM_RUN_CAP / SUM_BLK), a.runCap, lane);
      pile_sync();   // (the next peak's runs overwrite these)
    }
  }
}

}  // namespace gx
