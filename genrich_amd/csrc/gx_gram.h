// gx_gram.h -- the samples' coverage bins reduced to what a Pearson matrix needs (gx_coverage_gram; no Genrich counterpart:
// the sums a multiBamSummary / plotCorrelation pass takes from a second reading of every BAM).
//
// x_s[b] = sample s's sum120 of bin b (gx_coverage.h), over all bins of the context.  For S samples and n bins
//     n_zero     = number of bins b with x_s[b] == 0 for every s
//     sum[s]     = sum over b of x_s[b]
//     gram[i][j] = sum over b of x_i[b] x_j[b]
// as exact unsigned 128-bit integers.  With x < 2^51 (a bin of at most 2^20 bases under a pileup of at most 2^31 - 1) and
// sum of w_b^2 <= W G <= 2^64 (the host refuses more) every sum stays below 2^126.  No floating point, no atomics: a result does
// not depend on the grid or on the number of contexts.
//
// k_gram: grid (gx, nPairs + 1).  The pair matrix is cut into GRAM_T x GRAM_T sample tiles; blockIdx.y numbers the tiles
// (I, J), I <= J, row by row, and a workgroup streams the rows of its two sample tiles -- lane l of the grid's x axis takes
// bins l, l + stride, ..: one coalesced 8-byte load per row and bin -- into GRAM_T^2 128-bit accumulators per lane (a tile on
// the diagonal: its upper half, and one tile's rows only).  The tiles (0, J) also keep the sums of tile J's samples.  The
// workgroups of the last blockIdx.y count the all-zero bins over all S rows.  Every product is the full 64 x 64 -> 128
// (a wave-uniform 32 x 32 step for small values was tried and is not kept: its gain was never measured).
// At the end lane -> wavefront by shuffles of the two halves, wavefront -> workgroup through LDS, every add 128 bits wide;
// the workgroup stores its GRAM_ACCS sums to partial[blockIdx.y][blockIdx.x][.] with plain stores.
// k_gram_sum: out[y][a] = sum over x of partial[y][x][a], one workgroup per y.
#pragma once
#include "gx_coverage.h"

namespace gx {

typedef unsigned __int128 u128;

constexpr int GRAM_T = 4;                                   // samples along a tile's edge
constexpr int GRAM_NW = 4;                                  // wavefronts per workgroup
constexpr int GRAM_ACCS = GRAM_T * GRAM_T + GRAM_T + 1;     // a workgroup's results: the pairs, the sums, the zero bins
constexpr u32 GRAM_MAX_S = 32;                              // most samples
constexpr u32 GRAM_GRID = 1024;                             // most workgroups along the bin axis unless the caller says so
constexpr u32 GRAM_MAX_GRID = 65535;                        // ... and the most a caller may force (gx_gram_u64)
// (gx_gram_geometry reports GRAM_T, GRAM_NW * 64 and GRAM_GRID: the tests take the edges they probe from it)

__device__ __forceinline__ u128 gram_wave_sum(u128 v) {   // (lane 0 has the wavefront's sum)
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const unsigned long long lo = __shfl_down((unsigned long long)v, off, 64);
    const unsigned long long hi = __shfl_down((unsigned long long)(v >> 64), off, 64);
    v += ((u128)hi << 64) | lo;
  }
  return v;
}

__global__ __launch_bounds__(GRAM_NW * 64) void k_gram(const unsigned long long* const* __restrict__ rows, u32 S, u64 n, u32 nTiles,
                                                       unsigned long long* __restrict__ partial /* [gridDim.y][gridDim.x][GRAM_ACCS][2] */) {
  __shared__ unsigned long long red[GRAM_NW][GRAM_ACCS][2];
  const int wv = threadIdx.x >> 6, lane = lane_id();
  const u64 stride = (u64)gridDim.x * (GRAM_NW * 64);
  const u64 first = ((u64)blockIdx.x * GRAM_NW + wv) * 64;
  u128 acc[GRAM_T][GRAM_T], sum[GRAM_T];
  unsigned long long zeros = 0;
#pragma unroll
  for (int i = 0; i < GRAM_T; i++) {
    sum[i] = 0;
#pragma unroll
    for (int j = 0; j < GRAM_T; j++) acc[i][j] = 0;
  }
  if (blockIdx.y + 1 == gridDim.y) {   // the all-zero bins
    for (u64 b = first + lane; b < n; b += stride) {
      unsigned long long any = 0;
      for (u32 s = 0; s < S; s++) any |= rows[s][b];
      zeros += any == 0;
    }
  } else {
    u32 I = 0, r = blockIdx.y;
    while (r >= nTiles - I) {
      r -= nTiles - I;
      I++;
    }
    const u32 J = I + r;
    const bool diag = I == J, sums = I == 0;
    const unsigned long long* ra[GRAM_T];
    const unsigned long long* rb[GRAM_T];
#pragma unroll
    for (int i = 0; i < GRAM_T; i++) {   // (nullptr: the tile reaches past the last sample)
      ra[i] = I * GRAM_T + i < S ? rows[I * GRAM_T + i] : nullptr;
      rb[i] = J * GRAM_T + i < S ? rows[J * GRAM_T + i] : nullptr;
    }
    for (u64 b = first + lane; b < n; b += stride) {   // (the last step of a wavefront may be a part of its lanes)
      unsigned long long a[GRAM_T], c[GRAM_T];
#pragma unroll
      for (int i = 0; i < GRAM_T; i++) {
        a[i] = ra[i] ? ra[i][b] : 0ull;
      }
#pragma unroll
      for (int j = 0; j < GRAM_T; j++) {
        c[j] = diag ? a[j] : (rb[j] ? rb[j][b] : 0ull);
      }
      if (sums) {
#pragma unroll
        for (int j = 0; j < GRAM_T; j++) sum[j] += c[j];
      }
#pragma unroll
      for (int i = 0; i < GRAM_T; i++)
#pragma unroll
        for (int j = 0; j < GRAM_T; j++)
          if (ra[i] && rb[j] && (!diag || j >= i)) acc[i][j] += (u128)a[i] * (u128)c[j];
    }
  }
  // (every wavefront gets here)
#pragma unroll
  for (int i = 0; i < GRAM_T; i++)
#pragma unroll
    for (int j = 0; j < GRAM_T; j++) {
      const u128 v = gram_wave_sum(acc[i][j]);
      if (lane == 0) {
        red[wv][i * GRAM_T + j][0] = (unsigned long long)v;
        red[wv][i * GRAM_T + j][1] = (unsigned long long)(v >> 64);
      }
    }
#pragma unroll
  for (int j = 0; j < GRAM_T; j++) {
    const u128 v = gram_wave_sum(sum[j]);
    if (lane == 0) {
      red[wv][GRAM_T * GRAM_T + j][0] = (unsigned long long)v;
      red[wv][GRAM_T * GRAM_T + j][1] = (unsigned long long)(v >> 64);
    }
  }
  {
    const u128 v = gram_wave_sum((u128)zeros);
    if (lane == 0) {
      red[wv][GRAM_ACCS - 1][0] = (unsigned long long)v;
      red[wv][GRAM_ACCS - 1][1] = (unsigned long long)(v >> 64);
    }
  }
  __syncthreads();
  if (threadIdx.x < GRAM_ACCS) {
    u128 s = 0;
#pragma unroll
    for (int w = 0; w < GRAM_NW; w++) s += ((u128)red[w][threadIdx.x][1] << 64) | red[w][threadIdx.x][0];
    unsigned long long* out = partial + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * GRAM_ACCS + threadIdx.x) * 2;
    out[0] = (unsigned long long)s;
    out[1] = (unsigned long long)(s >> 64);
  }
}

// out[y][a] = sum over x of partial[y][x][a]: a workgroup per y, eight groups of partials
__global__ __launch_bounds__(256) void k_gram_sum(const unsigned long long* __restrict__ partial, u32 nPart,
                                                  unsigned long long* __restrict__ out /* [gridDim.x][GRAM_ACCS][2] */) {
  __shared__ unsigned long long red[8][GRAM_ACCS][2];
  const u32 a = threadIdx.x & 31, g = threadIdx.x >> 5;
  if (a < GRAM_ACCS) {
    u128 s = 0;
    for (u32 p = g; p < nPart; p += 8) {
      const unsigned long long* in = partial + (((size_t)blockIdx.x * nPart + p) * GRAM_ACCS + a) * 2;
      s += ((u128)in[1] << 64) | in[0];
    }
    red[g][a][0] = (unsigned long long)s;
    red[g][a][1] = (unsigned long long)(s >> 64);
  }
  __syncthreads();
  if (threadIdx.x < GRAM_ACCS) {
    u128 s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += ((u128)red[k][threadIdx.x][1] << 64) | red[k][threadIdx.x][0];
    out[((size_t)blockIdx.x * GRAM_ACCS + threadIdx.x) * 2] = (unsigned long long)s;
    out[((size_t)blockIdx.x * GRAM_ACCS + threadIdx.x) * 2 + 1] = (unsigned long long)(s >> 64);
  }
}

}  // namespace gx
