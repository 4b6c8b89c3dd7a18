// gx_profile.h -- a sample's run-length pileup summed over strand-oriented windows around anchor sites (gx_set_profile; no
// Genrich counterpart: the integral gx_coverage.h takes over fixed genome-wide bins, taken around given positions instead).
//
// An anchor is (chrom, pos, strand) with strand +1 or -1.  With the flank F and the bin size B (B >= 1, F % B == 0) an anchor
// has nb = 2 F / B bins (nb <= 1024).  Bin j (0 <= j < nb) covers these bases x of the anchor's chromosome:
//     strand +:  pos - F + j B       <= x <  pos - F + (j + 1) B
//     strand -:  pos + F - (j + 1) B <  x <= pos + F - j B            (the mirror image)
// so that on both strands the anchor base is the first base, in reading direction, of bin nb / 2.
// cell120[a][j] = sum over the bases of bin j of anchor a of the sample's pileup there, in 1/120 units, an exact int64; the
// pileup is the one gx_get_coverage integrates (a treatment's `experimental` pileup; a control's own raw pileup, before factor
// and lambda; 0 inside -E regions: V_MARK intervals count 0).  Bases x < 0 or x >= len count 0 (the window arithmetic is
// 64-bit signed); an anchor with pos >= len covers whatever part of its window lies inside the chromosome.  A row is all zeros
// when the anchor's chromosome is skipped (-e), empty, not owned by this context (gx_set_owned), left out by the replicate's
// save mask, or behind the table (chrom >= nChrom).  agg120[j] = sum of cell120[a][j] over all anchors.  All of it integers:
// a result does not depend on the grid, on the order of the adds or on the number of contexts.
//
// k_profile is anchor-centric: a tile-centric pass would have to find the anchors of its tile, and 20,000 windows of 4,000
// bases touch 40,000 of hg38's 750,000 tiles.  One wavefront per anchor, grid-strided.  The host has resolved the first tile
// of the anchor's chromosome (layout_tiles knows it: no search here); the window [lo, hi), clipped to [0, len), overlaps the
// tiles lo / TILE .. (hi - 1) / TILE of it.  Each of them is walked piece by piece (gx_pileup.h says what a tile's pieces
// are, in both forms of the pileup), and every piece, clipped to the window, is the FOUR adds of gx_coverage.h into a
// per-wavefront LDS strip of nb + 2 bin-to-bin differences whose origin is the window's start and whose width is B.  A 64-bit
// wave scan of the strip is the row in ascending coordinates; for strand - it is read back mirrored, so that the stores of a
// row are coalesced on both strands.
// The aggregate costs no atomic: a wavefront keeps the sum of the rows it has made in registers (nb / 64 <= 16 words a lane),
// the wavefronts of a workgroup add theirs through the strips when their anchors are done, and the workgroup stores one row
// of `partial`, which k_profile_sum adds up column by column.
// LDS: PROF_NW strips of 1026 words = 32,832 bytes, static.
#pragma once
#include "gx_pileup.h"

namespace gx {

constexpr int PROF_NW = 4;                  // wavefronts per workgroup
constexpr u32 PROF_MAX_NB = 1024;           // most bins of an anchor
constexpr int PROF_SLOTS = PROF_MAX_NB / 64;   // ... per lane
constexpr u32 PROF_MAX_F = 1u << 20;        // largest flank
constexpr u64 PROF_MAX_CELLS = 1ull << 26;  // most cells of a kept matrix

struct ProfAnchor {
  u32 tile0;   // first tile of the anchor's chromosome; NULL_TILE: the context does not compute it (a row of zeros)
  u32 pos;
  int strand;  // +1 / -1
  u32 len;     // the chromosome's length
};

__global__ __launch_bounds__(PROF_NW * 64) void k_profile(PileIn in, u32 nTiles, const ProfAnchor* __restrict__ anchors, u32 nAnchors,
                                                          u32 F, u32 B, u32 nb, unsigned long long* __restrict__ cells /* or null */,
                                                          unsigned long long* __restrict__ partial /* [gridDim.x][nb] */) {
  __shared__ unsigned long long strip[PROF_NW][PROF_MAX_NB + 2];
  const int wv = threadIdx.x >> 6, lane = lane_id();
  unsigned long long* D = strip[wv];
  unsigned long long acc[PROF_SLOTS];
#pragma unroll
  for (int k = 0; k < PROF_SLOTS; k++) acc[k] = 0;
  const u32 stride = gridDim.x * PROF_NW;
  for (u32 a = blockIdx.x * PROF_NW + wv; a < nAnchors; a += stride) {   // (everything about an anchor is wave-uniform)
    const ProfAnchor A = anchors[a];
    const long long lo = (long long)A.pos - (long long)F + (A.strand < 0 ? 1 : 0), hi = lo + 2ll * (long long)F;
    const long long clo = lo < 0 ? 0 : lo, chi = hi < (long long)A.len ? hi : (long long)A.len;
    unsigned long long* row = cells ? cells + (size_t)a * nb : nullptr;
    if (A.tile0 == NULL_TILE || clo >= chi) {
      if (row)
        for (u32 j = lane; j < nb; j += 64) row[j] = 0;
      continue;
    }
    for (u32 j = lane; j < nb + 2; j += 64) D[j] = 0;
    pile_sync();
    const u32 t1 = A.tile0 + (u32)((chi - 1) >> TB);
    for (u32 t = A.tile0 + (u32)(clo >> TB); t <= t1 && t < nTiles; t++) {
      const TileMeta m = in.meta[t];
      if (!(m.flags & TM_ACTIVE) || m.pos0 >= m.len) continue;
      const u32 pos0 = m.pos0, tEnd = m.len - pos0 < (u32)TILE ? m.len : pos0 + (u32)TILE;
      const u32 wlo = max(pos0, (u32)clo), whi = min(tEnd, (u32)chi);
      if (wlo >= whi) continue;
      const u32 ao = in.tileIvOff[t], n = in.tileIvOff[t + 1] - ao;
      const bool lastTile = (m.flags & TM_LAST) != 0;   // (it ends the chromosome-closing interval: no tail)
      u32 a0 = ao;
      int tailV = 0;
      if (in.loose) {
        a0 = m.slot;
        if (!lastTile && t + 1 < nTiles) tailV = in.meta[t + 1].carry;
      } else if (!lastTile)
        tailV = in.v[ao + n];   // (a later tile of the chromosome ends it)
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
          const u32 rs = (u32)((long long)s - lo), re = (u32)((long long)e - lo);   // (0 <= rs < re <= 2 F <= 2^21)
          const u32 bs = rs / B, be = (re - 1) / B;                                 // (be < nb)
          const long long vv = v;
          if (bs == be) {
            const unsigned long long c = (unsigned long long)(vv * (long long)(re - rs));
            atomicAdd(&D[bs], c);
            atomicAdd(&D[bs + 1], 0ull - c);
          } else {
            const unsigned long long vw = (unsigned long long)(vv * (long long)B);
            const unsigned long long cs = (unsigned long long)(vv * (long long)((bs + 1) * B - rs));
            const unsigned long long ce = (unsigned long long)(vv * (long long)(re - be * B));
            atomicAdd(&D[bs], cs);
            atomicAdd(&D[bs + 1], vw - cs);
            atomicAdd(&D[be], ce - vw);
            atomicAdd(&D[be + 1], 0ull - ce);
          }
        }
        if (prevEnd >= whi) break;   // (the pieces ascend: the rest of the tile lies behind the window)
      }
    }
    pile_sync();
    unsigned long long run = 0;
    for (u32 j0 = 0; j0 < nb; j0 += 64) {
      const u32 j = j0 + lane;
      unsigned long long x = j < nb ? D[j] : 0ull;
      x = wave_incl_scan(x) + run;
      run = __shfl(x, 63, 64);
      if (j < nb) D[j] = x;
    }
    pile_sync();
#pragma unroll
    for (int k = 0; k < PROF_SLOTS; k++) {
      const u32 j = (u32)k * 64 + lane;
      if (j < nb) {
        const unsigned long long x = D[A.strand < 0 ? nb - 1 - j : j];
        if (row) row[j] = x;
        acc[k] += x;
      }
    }
    pile_sync();
  }
  // (every wavefront gets here: the grid-stride loop has no other exit)
#pragma unroll
  for (int k = 0; k < PROF_SLOTS; k++) {
    const u32 j = (u32)k * 64 + lane;
    if (j < nb) D[j] = acc[k];
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < nb; j += PROF_NW * 64) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < PROF_NW; w++) s += strip[w][j];
    partial[(size_t)blockIdx.x * nb + j] = s;
  }
}

// agg[j] = sum over k_profile's workgroups of partial[.][j]: 64 columns and four groups of rows per workgroup
__global__ __launch_bounds__(256) void k_profile_sum(const unsigned long long* __restrict__ partial, u32 nPart, u32 nb,
                                                     unsigned long long* __restrict__ agg) {
  __shared__ unsigned long long red[4][64];
  const u32 l = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + l;
  unsigned long long s = 0;
  if (j < nb)
    for (u32 p = g; p < nPart; p += 4) s += partial[(size_t)p * nb + j];
  red[g][l] = s;
  __syncthreads();
  if (g == 0 && j < nb) agg[j] = red[0][l] + red[1][l] + red[2][l] + red[3][l];
}

}  // namespace gx
