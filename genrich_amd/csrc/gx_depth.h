// gx_depth.h -- the distribution of per-base depth of a sample's run-length pileup (gx_set_depth_hist; no Genrich counterpart:
// what deepTools' plotCoverage estimates from sampled positions, what `samtools depth | awk` or mosdepth's distribution file
// take from another reading of the BAM).  (a part of gx_api.hip's translation unit)
//
// Every base outside the -E regions has a pileup v >= 0 in 1/120 units, the one k_cov_bins integrates.  Its whole depth is
// d = v div 120, its remainder r = v mod 120 (non-zero only with -s weights).  Wanted, over the bases with v > 0:
//   d < DEPTH_BOUND:  bases[d], rsum[d] = sum of r, rsq[d] = sum of r^2     (class 0 holds 0 < v < 120)
//   d >= DEPTH_BOUND: the deep list, (v, bases) with the exact v
// and the smallest and the largest v met.  The bases at v = 0 are the host's complement (gx_host_depth.h): the tiles of a
// chromosome the replicate's header does not list are never visited, as in k_cov_bins.
//
// k_depth_hist is tile-centric, one wavefront per tile, and walks a tile's pieces (gx_pileup.h says what they are, in both
// forms of the pileup).  A piece [s, e) of pileup v is ONE add of e - s to bases[d] of the workgroup's LDS table (and one each
// to rsum / rsq when r != 0).
// Contention: nearly every piece of a real track has d in 1 .. DEPTH_PRIV and r == 0, and their adds meet on DEPTH_PRIV LDS
// words.  Measured against it (PRIV = true, GX_DEPTH_PRIV): those pieces summed in DEPTH_PRIV registers per lane, reduced over
// the wavefront once, after its last tile, and added to LDS with one atomic per class and wavefront.  It gains nothing at
// benchmark size (the pass waits for each tile's dependent loads, not for LDS), so the plain adds are the
// default.
// LDS counters: bases[] is 32-bit.  A wavefront walks at most DEPTH_WAVE_TILES tiles (the host sizes the grid for it), a tile
// has at most TILE bases: a workgroup adds at most DEPTH_NW * DEPTH_WAVE_TILES * TILE = 2^31 bases to its table, a lane's
// registers (PRIV) at most 2^28.  rsum[] and rsq[] are 64-bit (r^2 < 2^14: 32 bits would hold 74 tiles).
// The table is flushed with 64-bit global adds for its non-empty entries, as k_fp_hist does.  It is 40 KiB: four workgroups,
// all 32 wavefronts, per CU.
// Deep pieces are appended with one global counter add per wavefront and step (ballot + popcount), as k_cpx_hist appends its
// `big` list.  When the list is full the kernel keeps counting the entries it would have written and raises DEPTH_ST_LIST_FULL:
// the host reallocates to the counted size and runs the pass once more.  No workgroup waits for another; every loop is bounded.
// All of it integers: the result does not depend on the grid, the list's capacity or the order of the adds.
#pragma once
#include "gx_pileup.h"

namespace gx {

constexpr int DEPTH_NW = 8;                   // wavefronts per workgroup
constexpr u32 DEPTH_BOUND = 2048;             // whole depths below it are counted in LDS, the others listed
constexpr u32 DEPTH_PRIV = 4;                 // PRIV: classes 1 .. DEPTH_PRIV with r == 0 are summed in registers
constexpr u32 DEPTH_WAVE_TILES = 1u << 16;    // most tiles one wavefront walks (the 32-bit LDS counters' bound)
constexpr u32 DEPTH_LIST_CAP = 1u << 16;      // entries of the deep list at first
constexpr u32 DEPTH_GRID = 1024;             // most workgroups unless the caller says so: four per CU, all its wavefronts
constexpr u32 DEPTH_MAX_GRID = 65535;         // ... and the most a caller may force

// the control words (u64), ahead of bases[DEPTH_BOUND], rsum[DEPTH_BOUND], rsq[DEPTH_BOUND]
enum { DPC_NDEEP = 0, DPC_STATUS = 1, DPC_VMAX = 2, DPC_VMININV = 3 /* max of ~v over the pieces */, DPC_WORDS = 4 };
enum { DEPTH_ST_LIST_FULL = 1, DEPTH_ST_NEGATIVE = 2 };

struct DepthDeep { u32 v, bases; };   // one deep piece

template <bool PRIV>
__global__ __launch_bounds__(DEPTH_NW * 64) void k_depth_hist(PileIn in, u32 nTiles, unsigned long long* __restrict__ out,
                                                              DepthDeep* __restrict__ deep, u32 deepCap) {
  __shared__ u32 lb[DEPTH_BOUND];
  __shared__ unsigned long long lr[DEPTH_BOUND], lq[DEPTH_BOUND];
  for (u32 k = threadIdx.x; k < DEPTH_BOUND; k += DEPTH_NW * 64) {
    lb[k] = 0;
    lr[k] = 0;
    lq[k] = 0;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = lane_id();
  const u32 stride = gridDim.x * DEPTH_NW;
  u32 priv[DEPTH_PRIV] = {};
  u32 vmax = 0, vmininv = 0, stat = 0;
  for (u32 t = blockIdx.x * DEPTH_NW + wv; t < nTiles; t += stride) {   // (everything about a tile is wave-uniform)
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
    if (in.tileChrom[t] >= in.nChrom) continue;
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
      const bool live = i <= n && s < e && v != 0 && v != V_MARK;
      if (live && v < 0) stat |= DEPTH_ST_NEGATIVE;   // (no pileup is: the host says GX_ERR_DEVICE)
      const bool piece = live && v > 0;
      const u32 uv = (u32)v, len = e - s, d = uv / 120u, r = uv - d * 120u;
      if (piece) {
        vmax = max(vmax, uv);
        vmininv = max(vmininv, ~uv);
        if (PRIV && r == 0 && d - 1u < DEPTH_PRIV) {
#pragma unroll
          for (u32 k = 0; k < DEPTH_PRIV; k++) priv[k] += d == k + 1 ? len : 0u;
        } else if (d < DEPTH_BOUND) {
          atomicAdd(&lb[d], len);
          if (r) {
            atomicAdd(&lr[d], (unsigned long long)r * len);
            atomicAdd(&lq[d], (unsigned long long)(r * r) * len);
          }
        }
      }
      const unsigned long long heavy = __ballot(piece && d >= DEPTH_BOUND);
      if (heavy) {
        u32 first = 0;
        if (lane == 0) first = (u32)atomicAdd(&out[DPC_NDEEP], (unsigned long long)__popcll(heavy));
        first = (u32)__shfl((int)first, 0, 64);
        if (piece && d >= DEPTH_BOUND) {
          const u32 at = first + (u32)__popcll(heavy & ((1ull << lane) - 1));
          if (at < deepCap) deep[at] = DepthDeep{uv, len};
          else stat |= DEPTH_ST_LIST_FULL;
        }
      }
    }
  }
  if (PRIV) {
#pragma unroll
    for (u32 k = 0; k < DEPTH_PRIV; k++) {
      u32 x = priv[k];
      for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
      if (lane == 0 && x) atomicAdd(&lb[k + 1], x);
    }
  }
  for (int o = 32; o; o >>= 1) {   // (the extremes and the status: one global atomic each per wavefront that has something to say)
    vmax = max(vmax, (u32)__shfl_xor((int)vmax, o, 64));
    vmininv = max(vmininv, (u32)__shfl_xor((int)vmininv, o, 64));
    stat |= (u32)__shfl_xor((int)stat, o, 64);
  }
  if (lane == 0) {
    if (vmax) atomicMax(&out[DPC_VMAX], (unsigned long long)vmax);
    if (vmininv) atomicMax(&out[DPC_VMININV], (unsigned long long)vmininv);
    if (stat) atomicOr(&out[DPC_STATUS], (unsigned long long)stat);
  }
  __syncthreads();
  for (u32 k = threadIdx.x; k < DEPTH_BOUND; k += DEPTH_NW * 64) {
    if (lb[k]) atomicAdd(&out[DPC_WORDS + k], (unsigned long long)lb[k]);
    if (lr[k]) atomicAdd(&out[DPC_WORDS + DEPTH_BOUND + k], lr[k]);
    if (lq[k]) atomicAdd(&out[DPC_WORDS + 2 * DEPTH_BOUND + k], lq[k]);
  }
}

}  // namespace gx
