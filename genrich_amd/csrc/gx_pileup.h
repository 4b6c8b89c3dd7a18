// gx_pileup.h -- the closed sample's run-length pileup as every pass over it reads it, tile by tile (k_cov_bins, k_depth_hist,
// k_profile; the pileup's counterpart of gx_kept.h).  (a part of gx_api.hip's translation unit)
//
// A sample's pileup is a list of intervals (end, v) in ascending coordinates: v, in 1/120 units (V_MARK inside -E regions),
// holds from the previous interval's end up to `end`.  It lies in one of two forms (pile_input, gx_host_coverage.h, says which):
//   loose slots   where close_sample left them: tile t's intervals from meta[t].slot on
//   tight arrays  (pack_pileup; with -E regions): tile t's intervals from tileIvOff[t] on, side by side over the tiles
// and in both tile t ends n = tileIvOff[t + 1] - tileIvOff[t] intervals.  One wavefront accounts for an active tile's own bases
// [pos0, tEnd), tEnd = min(pos0 + TILE, len), as n + 1 PIECES [s, e) of pileup v: piece i < n is interval i, from the end of the
// one before it, the first clipped at pos0; the last one is the tail behind the tile's last breakpoint, up to tEnd, at the pileup
// of the interval that a later tile ends (loose slots: the next tile's carry -- no breakpoint lies between; tight arrays: the
// next interval itself, where no carry says V_MARK).  The chromosome's last tile (TM_LAST) ends the chromosome-closing
// interval: it has no tail.  Pieces with v == 0 or V_MARK count nothing anywhere.
// The walk over the pieces stands in each of the three kernels (profiles/r28_pileup_walk.txt); tests/test_hip_pileup_walk.py
// holds the three copies to the same constructed tiles.
#pragma once
#include "gx_kernels.h"

namespace gx {

struct PileIn {
  const u32* end;          // interval ends (chromosome coordinates) and pileups (1/120 units, V_MARK inside -E regions):
  const int* v;            // the sample's loose slots, or its tight arrays
  const u32* tileIvOff;    // [nTiles + 1] tight offsets: tile t ends tileIvOff[t + 1] - tileIvOff[t] intervals
  const TileMeta* meta;    // pos0 / len / flags of every tile; loose: tile t's first slot, and the pileup of its tail in
                           // meta[t + 1].carry (no breakpoint lies between)
  const u32* tileChrom;    // [nTiles] the tile's chromosome (k_sbtile's descriptors do not carry it)
  u32 loose;               // 0: tight arrays (tile t's intervals start at tileIvOff[t]; with -E regions: no carry says V_MARK)
  const u32* chromBin;     // the coverage's, set by its caller: [nChrom + 1] first bin of each chromosome in `bins`; [nChrom]: all bins
  u32 nChrom;
};

__device__ __forceinline__ void pile_sync() {  // (LDS operations of one wavefront execute in order: keep the compiler from reordering them)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace gx
