// gx_regions.h -- each kept sample's intervals counted in a caller's region set (gx_count_in_regions).  The regions may overlap,
// nest, repeat and come in any order, so gx_count.h's difference array over a sorted, disjoint list does not apply.
// (a part of gx_api.hip's translation unit; the intervals and the pass over them are gx_kept.h's)
//
// Coordinates are the context's tile space (gx_kept.h); a region's end is clamped to its chromosome's length, so it never
// reaches the next chromosome's tiles.  The m regions that can count anything ("live": a chromosome this context works on, start
// below its length) give A = their sorted starts and B = their sorted ends.  Per interval [s, e) with s <= e:
//   a = #{A < e}, b = #{B <= s}.  A region that ends at or before s starts before e, so the b regions are among the a, and the
//   interval overlaps exactly a - b regions: some region iff a > b.
// Region k at rank i in A and rank j in B is overlapped iff a > i and b <= j, and a <= i implies b <= j, so
//   count[k] = W{b <= j} - W{a <= i} = PB[j] - PA[i],
// PA / PB the inclusive prefix sums of two histograms HA[a] += w, HB[b] += w.  An interval with a == b overlaps nothing and adds
// the same amount to both terms of every region: it is left out.  Ties need no care: equal starts are all < e or none is.
// An inverted interval (e < s; gx_kept.h lets them in) breaks "the b regions are among the a": those go to a short list and
// are tested against every region directly (k_reg_inverted) after the gather.
// The histograms of one sample are one array H of 2 (m + 1) entries (HA, then HB).  While H fits REG_WIN_MAX LDS windows of
// CNT_LDS_MAX entries -- one -- it is kept in LDS (gx_kept.h's window, as in k_cnt_count; a launch per window).
// A larger H takes 64-bit global atomics in ONE launch: only the intervals that overlap a region add anything, the adds spread
// over H as the regions spread over the genome, and a second pass over the events costs more than they do (DESIGN.md section 4,
// "Counting in regions": measured).  All sums are integers: no result depends on the order of the adds.
#pragma once
#include "gx_kept.h"
#include "gx_count.h"   // (CNT_LDS_MAX, k_cnt_scan)

namespace gx {

constexpr u32 REG_WIN_MAX = 1;           // LDS windows per sample; more entries than that: global atomics (GX_REG_WINDOWS)
constexpr u32 REG_INV_CAP = 1u << 14;    // inverted intervals listed per pass (more: the pass runs again with a longer list)
constexpr int REG_SCAN_ITEMS = 4;
constexpr u32 REG_SCAN_TILE = CNT_NT * REG_SCAN_ITEMS;   // entries one workgroup scans

struct RegInv { u64 s, e; u32 w, sample; };

// #{A < x} / #{A <= x} inside [lo, hi] (everything below lo counts, nothing from hi on does)
__device__ __forceinline__ u32 reg_rank_lt(const u64* __restrict__ A, u32 lo, u32 hi, u64 x) {
  while (lo < hi) {
    const u32 k = (lo + hi) >> 1;
    if (A[k] < x) lo = k + 1; else hi = k;
  }
  return lo;
}
__device__ __forceinline__ u32 reg_rank_le(const u64* __restrict__ B, u32 lo, u32 hi, u64 x) {
  while (lo < hi) {
    const u32 k = (lo + hi) >> 1;
    if (B[k] <= x) lo = k + 1; else hi = k;
  }
  return lo;
}

// The tile index: idx[t] = {#{A < t * TILE}, #{A < (t + 1) * TILE}, #{B <= t * TILE}, #{B <= (t + 1) * TILE}}, t = 0 .. nTiles
// (A[m] = B[m] = ~0).  For x in tile t the first pair bounds #{A < x} from both sides, the second #{B <= x}: an interval whose
// two ends lie in one tile -- most do -- needs one 16-byte load for both searches.
__global__ void k_reg_index(const u64* __restrict__ A, const u64* __restrict__ B, u32 m, u32 nIdx, uint4* __restrict__ idx) {
  for (u32 t = blockIdx.x * blockDim.x + threadIdx.x; t < nIdx; t += gridDim.x * blockDim.x) {
    const u64 x = (u64)t << TB, x1 = x + TILE;
    uint4 v;
    v.x = reg_rank_lt(A, 0, m, x);
    v.y = reg_rank_lt(A, v.x, m, x1);
    v.z = reg_rank_le(B, 0, m, x);
    v.w = reg_rank_le(B, v.z, m, x1);
    idx[t] = v;
  }
}

struct RegArgs {
  const CntChunk* chunks;
  u32 nChunks;
  const CntChrom* chroms;
  u32 nChrom;
  const u64* A;
  const u64* B;
  const uint4* idx;
  u32 m;                    // live regions
  u32 w0, wn;               // LDS: this launch's window of H, entries [w0, w0 + wn)
  unsigned long long* hist; // H [2 (m + 1)] (int64 two's complement)
  unsigned long long* tot;  // {total, in_regions}; null: another window's launch adds them and lists the inverted intervals
  RegInv* inv;              // [invCap]
  u32* nInv;
  u32 invCap;
  u32 sample;
};

template <bool LDS>
__global__ __launch_bounds__(CNT_NT) void k_reg_count(RegArgs a) {
  extern __shared__ int regLds[];
  __shared__ long long red[2][CNT_NT / 64];
  if (LDS) kept_window_clear(regLds, a.wn);
  long long tot = 0, inr = 0;
  kept_walk(a.chunks, a.nChunks, a.chroms, a.nChrom, [&](const KeptIv& v, int) {
    tot += v.w;
    if (v.e < v.s) {   // inverted: k_reg_inverted
      if (a.tot) {
        const u32 at = atomicAdd(a.nInv, 1u);
        if (at < a.invCap) a.inv[at] = RegInv{v.s, v.e, (u32)v.w, a.sample};
      }
      return;
    }
    const u32 ts = (u32)(v.s >> TB), te = (u32)(v.e >> TB);
    const uint4 is = a.idx[ts];
    uint2 ie = make_uint2(is.x, is.y);
    if (te != ts) ie = *reinterpret_cast<const uint2*>(a.idx + te);
    const u32 x = reg_rank_lt(a.A, ie.x, ie.y, v.e);
    u32 y = reg_rank_le(a.B, is.z, is.w, v.s);
    if (x == y) return;
    inr += v.w;
    y += a.m + 1;
    if (LDS) {
      if (x - a.w0 < a.wn) atomicAdd(&regLds[x - a.w0], v.w);
      if (y - a.w0 < a.wn) atomicAdd(&regLds[y - a.w0], v.w);
    } else {
      atomicAdd(a.hist + x, (unsigned long long)v.w);
      atomicAdd(a.hist + y, (unsigned long long)v.w);
    }
  });
  if (LDS) kept_window_flush(regLds, a.w0, a.wn, a.hist);
  if (!a.tot) return;
  tot = kept_block_sum(tot, red[0]);
  inr = kept_block_sum(inr, red[1]);
  if (threadIdx.x == 0) {
    if (tot) atomicAdd(a.tot, (unsigned long long)tot);
    if (inr) atomicAdd(a.tot + 1, (unsigned long long)inr);
  }
}

// The prefix sums of H's segments (2 per sample, seg entries apart, the first m entries of each), by tiles of REG_SCAN_TILE:
// the tiles' sums (k_reg_tile_sums), their prefix sums per segment (k_cnt_scan), the scan inside each tile (k_reg_tile_scan).

// sums[seg * (nT + 1) + tile]; grid (nT, segments)
__global__ __launch_bounds__(CNT_NT) void k_reg_tile_sums(const long long* __restrict__ H, u32 m, size_t seg, u32 nT,
                                                          long long* __restrict__ sums) {
  __shared__ long long sh[CNT_NT / 64];
  const long long* h = H + (size_t)blockIdx.y * seg;
  const u32 k0 = blockIdx.x * REG_SCAN_TILE + threadIdx.x * REG_SCAN_ITEMS;
  long long v = 0;
#pragma unroll
  for (int j = 0; j < REG_SCAN_ITEMS; j++)
    if (k0 + j < m) v += h[k0 + j];
  v = kept_block_sum(v, sh);
  if (threadIdx.x == 0) sums[(size_t)blockIdx.y * (nT + 1) + blockIdx.x] = v;
}

// in place: H[k] = sum of H[0 .. k] within its segment (k < m); pre[seg * (nT + 1) + tile] = inclusive prefix of the tile sums
__global__ __launch_bounds__(CNT_NT) void k_reg_tile_scan(long long* __restrict__ H, u32 m, size_t seg, u32 nT,
                                                          const long long* __restrict__ pre) {
  __shared__ long long sh[CNT_NT / 64];
  long long* h = H + (size_t)blockIdx.y * seg;
  const u32 k0 = blockIdx.x * REG_SCAN_TILE + threadIdx.x * REG_SCAN_ITEMS;
  long long v[REG_SCAN_ITEMS], sum = 0;
#pragma unroll
  for (int j = 0; j < REG_SCAN_ITEMS; j++) {
    v[j] = k0 + j < m ? h[k0 + j] : 0;
    sum += v[j];
  }
  long long inc = sum;   // inclusive scan of the threads' sums: inside the wave, then over the waves
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  long long run = blockIdx.x ? pre[(size_t)blockIdx.y * (nT + 1) + blockIdx.x - 1] : 0;
  for (int k = 0; k < wv; k++) run += sh[k];
  run += inc - sum;
#pragma unroll
  for (int j = 0; j < REG_SCAN_ITEMS; j++) {
    run += v[j];
    if (k0 + j < m) h[k0 + j] = run;
  }
}

// out[sample * stride + k] = PB[rankB[k]] - PA[rankA[k]] (0 for a region that is not live: rankA = ~0); grid (.., samples)
__global__ void k_reg_gather(const long long* __restrict__ P, u32 m, const u32* __restrict__ rankA,
                             const u32* __restrict__ rankB, u32 n, size_t stride, long long* __restrict__ out) {
  const long long* pa = P + (size_t)blockIdx.y * 2 * (m + 1);
  const long long* pb = pa + (m + 1);
  long long* o = out + (size_t)blockIdx.y * stride;
  for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const u32 i = rankA[k];
    o[k] = i == ~0u ? 0 : pb[rankB[k]] - pa[i];
  }
}

// the listed inverted intervals [s, e), e < s, against every region by the predicate itself (s < end && start < e); a workgroup
// per interval.  Adds to the gathered counts and to in_regions (out[sample * stride + n + 1]).
__global__ __launch_bounds__(CNT_NT) void k_reg_inverted(const RegInv* __restrict__ inv, const u32* __restrict__ nInv, u32 invCap,
                                                         const u64* __restrict__ A, const u64* __restrict__ B,
                                                         const u32* __restrict__ rankA, const u32* __restrict__ rankB, u32 n,
                                                         size_t stride, unsigned long long* __restrict__ out) {
  const u32 cnt = min(*nInv, invCap);
  for (u32 i = blockIdx.x; i < cnt; i += gridDim.x) {
    const RegInv v = inv[i];
    unsigned long long* o = out + (size_t)v.sample * stride;
    int hit = 0;
    for (u32 k = threadIdx.x; k < n; k += CNT_NT) {
      const u32 ra = rankA[k];
      if (ra == ~0u) continue;
      if (v.s < B[rankB[k]] && A[ra] < v.e) {
        atomicAdd(o + k, (unsigned long long)v.w);
        hit = 1;
      }
    }
    if (__syncthreads_or(hit) && threadIdx.x == 0) atomicAdd(o + n + 1, (unsigned long long)v.w);
  }
}

}  // namespace gx
