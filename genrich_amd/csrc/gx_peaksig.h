// gx_peaksig.h -- each kept sample's own depth inside the called peaks (gx_peak_signal): per (sample, peak) its area, its
// maximum, where it first reaches it, how many bases it covers and what it has at the run's summit base.  Genrich has no
// counterpart: a sample's pileup ends in the p-values and the replicates' p-values in Fisher's sum; the narrowPeak line does
// not say which replicate carries a peak.
// (a part of gx_api.hip's translation unit)
//
// The intervals, the pass over them, the peak list in tile space, its sentinel and its tile index are gx_kept.h's and
// gx_count.h's.  The samples' pileups are gone by the time the peaks are known, but inside the peaks (a few percent of the
// genome) they are cheap to make again: the peaks laid out back to back form the PEAK SPACE, one int32 per base, each peak's
// slots padded to a multiple of PSIG_PAD so that a lane's 16-byte load stays aligned; peak k's slots start at off[k] (u64).
// k_psig_scatter writes a sample's difference array into it: per interval [s, e) with weight w and per peak [ps, pe) it
// touches, +w at slot max(s, ps) - ps if s < pe and -w at slot max(e, ps) - ps if e < pe.  The one rule serves an interval
// inside a peak, one clipped at either edge, one that spans it (the -w falls behind the peak: not written), an empty one (no
// add at all) and one that ends before it starts (-w over [e, s), as in the pileup); slot pe - ps is never written.  The
// events come in no order, so the adds are global atomics (int32, return-less): a sum may wrap on its way, only the final
// entry must fit, and the pileup's own domain -- a depth below 2^31 at every base -- says it does.  k_psig_reduce gives one
// wavefront per peak: 4 slots per lane and step, the prefix sum in 64 bits, carried from step to step.  All figures are exact
// integers in 1/120 units: none depends on the grid or on the order of the adds.  The space is ONE buffer, cleared for every
// sample.
#pragma once
#include "gx_count.h"

namespace gx {

constexpr int PSIG_NT = 256;                  // k_psig_reduce: four wavefronts, a peak each
constexpr u32 PSIG_GRID = 2048;                // ... and at most so many workgroups of them, striding over the peaks
constexpr u32 PSIG_PAD = 4;                   // slots of a peak: a multiple of it (one int4 per lane)
constexpr u32 PSIG_STEP = 64 * PSIG_PAD;      // bases a wavefront covers per step

struct PsigRec { long long area, max, at; u32 summit, covered; };   // one (sample, peak)

struct PsigArgs {
  const CntChunk* chunks;
  u32 nChunks;
  const CntChrom* chroms;
  u32 nChrom;
  const CntPeak* pk;        // [nPk + 1], the sentinel last
  const u32* idx0;          // k_cnt_index
  const u64* off;           // [nPk] first slot of each peak
  int* space;
};

__global__ __launch_bounds__(CNT_NT) void k_psig_scatter(PsigArgs a) {
  kept_walk(a.chunks, a.nChunks, a.chroms, a.nChrom, [&](const KeptIv& v, int) {
    if (v.s == v.e) return;
    const u64 lo = min(v.s, v.e), hi = max(v.s, v.e);
    u32 k = a.idx0[lo >> TB];
    CntPeak P = a.pk[k];
    while (P.e <= lo) P = a.pk[++k];   // (the sentinel ends every scan)
    while (P.s < hi) {                 // the peaks with end > lo and start < hi
      int* row = a.space + a.off[k];
      if (v.s < P.e) atomicAdd(row + (max(v.s, P.s) - P.s), v.w);
      if (v.e < P.e) atomicAdd(row + (max(v.e, P.s) - P.s), -v.w);
      P = a.pk[++k];
    }
  });
}

// sumOff[k]: the base of peak k (from its start) whose depth goes into `at`
__global__ __launch_bounds__(PSIG_NT) void k_psig_reduce(const int* __restrict__ space, const u64* __restrict__ off, const CntPeak* __restrict__ pk,
                                                         const u32* __restrict__ sumOff, u32 nPk, PsigRec* __restrict__ out) {
  const u32 lane = threadIdx.x & 63u, wpb = PSIG_NT / 64;
  for (u32 k = blockIdx.x * wpb + (threadIdx.x >> 6); k < nPk; k += gridDim.x * wpb) {
    const CntPeak P = pk[k];
    const u64 L = P.e - P.s;
    const int4* row = reinterpret_cast<const int4*>(space + off[k]);
    const u64 so = sumOff[k];
    long long carry = 0, area = 0, mx = LLONG_MIN, at = 0;
    u32 pos = ~0u, cov = 0;
    for (u64 b = 0; b < L; b += PSIG_STEP) {
      const u64 x0 = b + lane * PSIG_PAD;
      int4 d = make_int4(0, 0, 0, 0);
      if (x0 < L) d = row[x0 >> 2];    // (the padding holds zeros)
      long long v[4];
      v[0] = d.x;
      v[1] = v[0] + d.y;
      v[2] = v[1] + d.z;
      v[3] = v[2] + d.w;
      long long incl = v[3];           // the wavefront's inclusive scan of the lanes' sums
      for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(incl, o);
        if (lane >= (u32)o) incl += t;
      }
      const long long before = carry + incl - v[3];
      carry += __shfl(incl, 63);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const u64 x = x0 + j;
        if (x >= L) break;
        const long long depth = before + v[j];
        area += depth;
        cov += depth > 0 ? 1u : 0u;
        if (depth > mx) {              // (ascending x: the first of equals stays)
          mx = depth;
          pos = (u32)x;
        }
        if (x == so) at = depth;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      area += __shfl_xor(area, o);
      cov += __shfl_xor(cov, o);
      at += __shfl_xor(at, o);
      const long long om = __shfl_xor(mx, o);
      const u32 op = __shfl_xor(pos, o);
      if (om > mx || (om == mx && op < pos)) {
        mx = om;
        pos = op;
      }
    }
    if (lane == 0) out[k] = PsigRec{area, mx, at, pos, cov};
  }
}

}  // namespace gx
