// gx_kept.h -- the kept samples' events as every pass over them reads them: gx_count.h (counts in peaks), gx_regions.h (counts
// in regions), gx_complexity.h (library complexity) and gx_subsample.h (subsamples) share what is here and nothing else.
// (a part of gx_api.hip's translation unit)
//
// A kept sample (gx_host_count.h keep_sample) reaches the device as a list of CntChunk -- up to CNT_CHUNK events each, all of
// one form: 16-byte gx_event, or 8-byte gx_event8 when packed -- and as its view of the chromosome table, one CntChrom per
// chromosome.  kept_event loads an event of either form as the four words of a gx_event; kept_interval is the ONE statement of
// which events are the sample's intervals, and where; kept_walk is the pass over a chunk list that three of the four make.
// Coordinates are the context's tile space: chromosome c's position x is tileBase(c) * TILE + x (gx_host_build.h layout_tiles).
#pragma once
#include "gx_sort.h"   // (unpack_event8)

namespace gx {

struct CntChrom { u64 base; u32 len; u32 active; };  // one sample's view of a chromosome (active: its events entered the pileup)
struct CntChunk { const void* p; u32 n; u32 packed; };  // up to CNT_CHUNK events of one sample (gx_event, or gx_event8 when packed)

constexpr int CNT_NT = 1024;
constexpr int CNT_ITEMS = 4;                  // events in flight per thread
constexpr u32 CNT_CHUNK = 1u << 16;
constexpr u32 CNT_WG_CHUNKS = 272;            // 120 * 272 * 2^16 < 2^31

// event i of a chunk, as the four words of a gx_event: chromosome, start, end, count
__device__ __forceinline__ uint4 kept_event(const CntChunk& ch, u32 i) {
  if (ch.packed) {
    const uint2 v = static_cast<const uint2*>(ch.p)[i];
    return unpack_event8(v.x, v.y);
  }
  return static_cast<const uint4*>(ch.p)[i];
}

// One interval of a sample: its weight in 1/120 units (0: the event is none of the sample's intervals), its start and its
// clamped end in tile space, and the first position of its chromosome there (s - base, e - base: the chromosome's own).
struct KeptIv { int w; u64 s, e, base; };

// an event's words, seen through the sample's chromosome views chroms[nChrom]
__device__ __forceinline__ KeptIv kept_interval(const uint4 ev, const CntChrom* __restrict__ chroms, u32 nChrom) {
  const u32 chrom = ev.x, s = ev.y, e = ev.z, cnt = ev.w;
  KeptIv iv{0, 0, 0, 0};
  // what convert_event (gx_sort.h) lets into the pileup, empty intervals included (saveInterval prints them, Genrich.c:2586-2588):
  // a count in {1, 2, 3, 4, 5, 6, 8, 10}, a chromosome of the table that the sample's pileup took, a start below its length.
  // One that ends before it starts is let in too, and keeps its end.
  const bool cntOk = cnt <= 10u && ((0x57Eu >> cnt) & 1u);
  if (!cntOk || chrom >= nChrom) return iv;
  const CntChrom cc = chroms[chrom];
  if (!cc.active || s >= cc.len) return iv;
  iv.w = (int)(120u / cnt);
  iv.base = cc.base;
  iv.s = cc.base + s;
  iv.e = cc.base + (e > cc.len ? cc.len : e);  // 2536-2544
  return iv;
}

// The pass over a chunk list: the workgroups (CNT_NT lanes) stride the chunks, a chunk goes by batches of CNT_NT * CNT_ITEMS
// events.  All CNT_ITEMS events of a lane are loaded and turned into intervals before any is used, so that many lines are in
// flight per lane; then stage(iv) sees the lane's whole batch (further loads that should be in flight together), then
// body(iv[j], j) each interval with a weight.
template <typename Stage, typename Body>
__device__ __forceinline__ void kept_walk(const CntChunk* __restrict__ chunks, u32 nChunks, const CntChrom* __restrict__ chroms,
                                          u32 nChrom, Stage stage, Body body) {
  for (u32 c = blockIdx.x; c < nChunks; c += gridDim.x) {
    const CntChunk ch = chunks[c];
    for (u32 b = 0; b < ch.n; b += CNT_NT * CNT_ITEMS) {
      KeptIv iv[CNT_ITEMS];
#pragma unroll
      for (int j = 0; j < CNT_ITEMS; j++) {
        const u32 i = b + (u32)j * CNT_NT + threadIdx.x;
        iv[j] = KeptIv{0, 0, 0, 0};
        if (i < ch.n) iv[j] = kept_interval(kept_event(ch, i), chroms, nChrom);
      }
      stage(iv);
#pragma unroll
      for (int j = 0; j < CNT_ITEMS; j++)
        if (iv[j].w) body(iv[j], j);
    }
  }
}
template <typename Body>
__device__ __forceinline__ void kept_walk(const CntChunk* __restrict__ chunks, u32 nChunks, const CntChrom* __restrict__ chroms,
                                          u32 nChrom, Body body) {
  kept_walk(chunks, nChunks, chroms, nChrom, [](const KeptIv(&)[CNT_ITEMS]) {}, body);
}

// a workgroup's (CNT_NT lanes) sum of v, in thread 0: inside the wavefronts, through sh[CNT_NT / 64], then thread 0 alone.
// Every lane of the workgroup calls it; two calls in flight take two arrays.
__device__ __forceinline__ long long kept_block_sum(long long v, long long* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < CNT_NT / 64; k++) t += sh[k];
  return t;
}

// A workgroup's LDS window over entries [w0, w0 + wn) of an array of 64-bit sums: int32 counters (a workgroup sees at most
// CNT_WG_CHUNKS chunks, 120 * CNT_WG_CHUNKS * CNT_CHUNK < 2^31), cleared before the walk, and after it one global add per
// non-zero counter.
__device__ __forceinline__ void kept_window_clear(int* lds, u32 wn) {
  for (u32 i = threadIdx.x; i < wn; i += CNT_NT) lds[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void kept_window_flush(const int* lds, u32 w0, u32 wn, unsigned long long* sums) {
  __syncthreads();
  for (u32 i = threadIdx.x; i < wn; i += CNT_NT) {
    const int v = lds[i];
    if (v) atomicAdd(sums + w0 + i, (unsigned long long)(long long)v);
  }
}

}  // namespace gx
