// gx_fingerprint.h -- the samples' coverage bins reduced to a histogram of value classes (gx_coverage_fingerprint; no Genrich
// counterpart: what a plotFingerprint pass takes from another reading of every BAM).
//
// x_s[b] = sample s's sum120 of bin b (gx_coverage.h), over all bins of the context.  With class() of gx_fp_class.h
//     count[s][k] = number of bins b with class(x_s[b]) == k
//     sum[s][k]   = the sum of those x_s[b]
// as exact uint64 (a sample's total stays below 2^64: the host refuses a genome of 2^33 bases or more).  Integer adds only:
// a result does not depend on the grid, on the order of the adds or on the number of contexts.
//
// k_fp_hist<AGG>: grid (gx, S), blockIdx.y = the sample.  A workgroup keeps one table of FP_NC classes in LDS -- a 32-bit
// count (a context has at most 2^30 bins) and a 64-bit sum each, 45,312 bytes: three workgroups per CU -- and streams its share
// of the row: a wavefront's step is 64 lanes x 16 bytes (two values a lane, the rows are 16-byte aligned), two steps loaded
// before the first is used.  Zeros never touch LDS: a zero adds nothing to a sum, so a step costs one ballot and one popcount
// per value slot, kept in a scalar and added to class 0 once per wavefront at the end.  The other values:
//     AGG = false  a 32-bit and a 64-bit LDS atomic per lane;
//     AGG = true   the lanes that hold one class elect a leader: per distinct class of the step one ballot, one sum over the
//                  wavefront by shuffles and one pair of atomics.
// (which of them runs: Knobs::fpAgg; DESIGN section 4, "Fingerprint of the samples' bins", has the two timings.)
// At the end the workgroup adds its non-empty classes to out[s][k] (count) and out[S + s][k] (sum) with 64-bit global
// atomics; the host zeroed the array with one fill.
#pragma once
#include "gx_coverage.h"

namespace gx {

constexpr int FP_NC = GX_FP_NC;          // value classes
constexpr int FP_NW = 8;                 // wavefronts per workgroup
constexpr u32 FP_MAX_S = 32;             // most samples
constexpr u32 FP_GRID = 768;             // most workgroups of a launch unless the caller says so: three per CU; with S samples
                                         // FP_GRID / S along the bin axis
constexpr u32 FP_MAX_GRID = 65535;       // ... and the most a caller may force along the bin axis (gx_fp_u64)
// (gx_fp_geometry reports FP_NC, GX_FP_SUB_LOG, FP_NW * 64 and FP_GRID: the tests take the edges they probe from it)

// one value slot of a wavefront's step: `have` = this lane holds a value of the row
template <bool AGG>
__device__ __forceinline__ void fp_add(unsigned long long v, bool have, int lane, u32& zeros, u32* hc, unsigned long long* hs) {
  const bool live = have && v != 0;
  zeros += (u32)__popcll(__ballot(have && v == 0));
  const u32 k = fp_class(v);
  if (!AGG) {
    if (live) {
      atomicAdd(&hc[k], 1u);
      atomicAdd(&hs[k], v);
    }
  } else {
    unsigned long long todo = __ballot(live);
    while (todo) {   // (wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const u32 kl = (u32)__shfl((int)k, leader, 64);
      const bool mine = live && k == kl;
      const unsigned long long same = __ballot(mine);
      const unsigned long long s = wave_sum(mine ? v : 0ull);   // (every lane has it)
      if (lane == leader) {
        atomicAdd(&hc[kl], (u32)__popcll(same));
        atomicAdd(&hs[kl], s);
      }
      todo &= ~same;
    }
  }
}

template <bool AGG>
__global__ __launch_bounds__(FP_NW * 64) void k_fp_hist(const unsigned long long* const* __restrict__ rows, u64 n,
                                                        unsigned long long* __restrict__ out /* [2][gridDim.y][FP_NC] */) {
  __shared__ unsigned long long hs[FP_NC];
  __shared__ u32 hc[FP_NC];
  for (u32 k = threadIdx.x; k < (u32)FP_NC; k += FP_NW * 64) {
    hs[k] = 0;
    hc[k] = 0;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = lane_id();
  const unsigned long long* row = rows[blockIdx.y];
  const ulonglong2* row2 = reinterpret_cast<const ulonglong2*>(row);
  const u64 n2 = n >> 1;                                              // pairs of values
  const u64 stride = (u64)gridDim.x * (FP_NW * 64);
  u32 zeros = 0;
  for (u64 base = ((u64)blockIdx.x * FP_NW + wv) * 64; base < n2; base += 2 * stride) {   // (wave-uniform: the ballots see 64 lanes)
    const u64 p0 = base + lane, p1 = p0 + stride;
    const bool h0 = p0 < n2, h1 = p1 < n2;
    ulonglong2 a = make_ulonglong2(0, 0), b = make_ulonglong2(0, 0);
    if (h0) a = row2[p0];
    if (h1) b = row2[p1];
    fp_add<AGG>(a.x, h0, lane, zeros, hc, hs);
    fp_add<AGG>(a.y, h0, lane, zeros, hc, hs);
    fp_add<AGG>(b.x, h1, lane, zeros, hc, hs);
    fp_add<AGG>(b.y, h1, lane, zeros, hc, hs);
  }
  if ((n & 1) && blockIdx.x == 0 && wv == 0)                          // the last value of a row of odd length
    fp_add<AGG>(lane == 0 ? row[n - 1] : 0ull, lane == 0, lane, zeros, hc, hs);
  if (lane == 0 && zeros) atomicAdd(&hc[0], zeros);
  __syncthreads();
  unsigned long long* oc = out + (size_t)blockIdx.y * FP_NC;
  unsigned long long* os = out + ((size_t)gridDim.y + blockIdx.y) * FP_NC;
  for (u32 k = threadIdx.x; k < (u32)FP_NC; k += FP_NW * 64) {
    const u32 c = hc[k];
    if (c) {
      atomicAdd(&oc[k], (unsigned long long)c);
      if (k) atomicAdd(&os[k], hs[k]);
    }
  }
}

}  // namespace gx
