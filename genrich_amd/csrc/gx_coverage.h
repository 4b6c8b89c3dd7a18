// gx_coverage.h -- binned coverage of a sample's run-length pileup (gx_set_coverage_bins; no Genrich counterpart:
// what -k prints per run-length interval, printPile Genrich.c:1697, summed over fixed-width bins).
//
// sum120[b] of a chromosome = sum over the bases of bin b = [b W, min((b + 1) W, len)) of the pileup there, in 1/120 units
// (0 inside -E regions: V_MARK intervals count 0), as an exact int64.
//
// k_cov_bins is tile-centric, like k_pack and k_merge2w: one wavefront per tile, which accounts for the tile's own bases
// piece by piece (gx_pileup.h says what a tile's pieces are, in both forms of the pileup).
// Every piece [s, e) of pileup v is FOUR adds into a per-wavefront LDS strip D of bin-to-bin differences, however many bins
// it spans -- with bs / be its first / last bin, cs / ce its share of those two and v W the share of every bin between:
//     D[bs] += cs;  D[bs + 1] += v W - cs;  D[be] += ce - v W;  D[be + 1] -= ce        (bs == be: D[bs] += c; D[bs + 1] -= c)
// -- and the tile's bins are the running sum of D (a 64-bit wave scan).  A bin that lies wholly inside the tile is written
// with a plain store; a bin shared with a neighbouring tile (W does not divide TILE, W > TILE, the chromosome's short last
// bin next to a tile edge) is added with a 64-bit atomic into the array, which the host zeroed.  All of it integers: the
// result does not depend on the order of the adds, on the grid or on the number of contexts.
// The strip holds COV_CAP bins: a whole tile's for W >= 8; a tile with more bins (W < 8) is done in passes of COV_CAP bins,
// each of which reads the tile's intervals again (from the L2).
#pragma once
#include "gx_pileup.h"

namespace gx {

constexpr int COV_NW = 4;               // wavefronts per workgroup
constexpr u32 COV_CAP = 520;            // bins per pass: TILE / 8 + 1 (a bin cut by the tile's first base), rounded up
constexpr u32 COV_MAX_W = 1u << 20;     // largest bin
constexpr u64 COV_MAX_BINS = 1ull << 30;  // ... and most bins of a context (the chromosomes' first bins are 32-bit)

__global__ __launch_bounds__(COV_NW * 64) void k_cov_bins(PileIn in, u32 nTiles, u32 W, unsigned long long* __restrict__ bins) {
  __shared__ unsigned long long strip[COV_NW][COV_CAP + 2];
  const int wv = threadIdx.x >> 6, lane = lane_id();
  unsigned long long* D = strip[wv];
  const u32 stride = gridDim.x * COV_NW;
  for (u32 t = blockIdx.x * COV_NW + wv; t < nTiles; t += stride) {   // (everything about a tile is wave-uniform)
    const TileMeta m = in.meta[t];
    if (!(m.flags & TM_ACTIVE) || m.pos0 >= m.len) continue;
    const u32 pos0 = m.pos0, tEnd = m.len - pos0 < (u32)TILE ? m.len : pos0 + (u32)TILE;
    const u32 ao = in.tileIvOff[t], n = in.tileIvOff[t + 1] - ao;
    const bool lastTile = (m.flags & TM_LAST) != 0;   // (it ends the chromosome-closing interval: no tail)
    u32 a0 = ao;
    int tailV = 0;
    if (in.loose) {
      a0 = m.slot;
      if (!lastTile && t + 1 < nTiles) tailV = in.meta[t + 1].carry;
    } else if (!lastTile)
      tailV = in.v[ao + n];   // (a later tile of the chromosome ends it)
    const u32 ci = in.tileChrom[t];
    if (ci >= in.nChrom) continue;
    const u64 bin0 = in.chromBin[ci], binEnd = in.chromBin[ci + 1];   // (no store beyond the chromosome's bins, whatever a descriptor says)
    const u32 b0 = pos0 / W, b1 = (tEnd - 1) / W;
    for (u64 wb64 = b0; wb64 <= b1; wb64 += COV_CAP) {
      const u32 wb = (u32)wb64, nb = min(COV_CAP, b1 - wb + 1);
      const u32 org = wb * W;   // (<= tEnd - 1: no wrap)
      const u32 wlo = max(pos0, org);
      const u32 whi = (u32)min((u64)org + (u64)nb * W, (u64)tEnd);
      for (u32 j = lane; j < nb + 2; j += 64) D[j] = 0;
      pile_sync();
      u32 prevEnd = pos0;
      for (u32 base = 0; base <= n; base += 64) {   // (piece n is the tail)
        const u32 i = base + lane;
        u32 e = tEnd;
        int v = tailV;
        if (i < n) {
          e = in.end[a0 + i];
          v = in.v[a0 + i];
        }
        e = min(max(e, pos0), tEnd);
        u32 s = __shfl_up(e, 1, 64);
        if (lane == 0) s = prevEnd;
        prevEnd = __shfl(e, 63, 64);
        s = max(s, wlo);
        e = min(e, whi);
        if (i <= n && s < e && v != 0 && v != V_MARK) {
          const u32 rs = s - org, re = e - org;         // (< COV_CAP W <= 2^30)
          const u32 bs = rs / W, be = (re - 1) / W;     // (be < nb)
          const long long vv = v;
          if (bs == be) {
            const unsigned long long c = (unsigned long long)(vv * (long long)(re - rs));
            atomicAdd(&D[bs], c);
            atomicAdd(&D[bs + 1], 0ull - c);
          } else {
            const unsigned long long vw = (unsigned long long)(vv * (long long)W);
            const unsigned long long cs = (unsigned long long)(vv * (long long)((bs + 1) * W - rs));
            const unsigned long long ce = (unsigned long long)(vv * (long long)(re - be * W));
            atomicAdd(&D[bs], cs);
            atomicAdd(&D[bs + 1], vw - cs);
            atomicAdd(&D[be], ce - vw);
            atomicAdd(&D[be + 1], 0ull - ce);
          }
        }
      }
      pile_sync();
      unsigned long long run = 0;
      for (u32 j0 = 0; j0 < nb; j0 += 64) {
        const u32 j = j0 + lane;
        unsigned long long x = j < nb ? D[j] : 0ull;
        x = wave_incl_scan(x) + run;
        run = __shfl(x, 63, 64);
        if (j < nb && bin0 + wb + j < binEnd) {
          const u32 b = wb + j;
          const u64 lo = (u64)b * W, hi = min(lo + W, (u64)m.len);
          if (lo >= pos0 && hi <= tEnd)
            bins[bin0 + b] = x;
          else if (x)
            atomicAdd(&bins[bin0 + b], x);
        }
      }
      pile_sync();
    }
  }
}

}  // namespace gx
