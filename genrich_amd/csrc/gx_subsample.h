// gx_subsample.h -- a deterministic, order-preserving subsample of a kept sample's events (gx_subsample_events,
// gx_subsample_kept, gx_saturation).  Genrich has no counterpart: a saturation curve re-runs the caller on `samtools view -s`
// subsamples of the BAM.
// (a part of gx_api.hip's translation unit)
//
// A sample's events are gx_kept.h's: the same chunk list, the same two event forms (kept_event).  Event i of the sample
// (its position in the chunk list's order, i.e. the kept order) is kept iff subsample_draw(key, i) < T (gx_math.h); the
// output is the kept events as 16-byte gx_event, in that order.  Every event is drawn, whatever its chromosome or count: the
// consumer applies its own rules, as the first run did.
//
// The events are cut into blocks of SUB_BLOCK: a chunk holds CNT_CHUNK / SUB_BLOCK of them (a chunk's last blocks may be
// short or empty), so block b is block b % SUB_BPC of chunk b / SUB_BPC and nothing has to be searched.
// 1. k_sub_count: the kept events per block.  The draw needs the index alone: no event is read.
// 2. k_sub_scan: one workgroup turns the counts into offsets (and the total behind the last).
// 3. k_sub_write: the draws once more; an event's rank inside its block is the kept events of the rows before its own (a row
//    = the SUB_NT events the lanes load together), of the wavefronts before its own in that row, and of the lanes before its
//    own by ballot and popcount; it is stored at block offset + rank.
// No workgroup waits for another: three launches, ordered by the stream.  Every loop is bounded by the chunk list.  An event's
// place depends on the block offsets alone, so the output is the same bytes for every grid.
// SUB_ITEMS = 8: the write pass is a streaming read whose only arithmetic is the draw; eight independent 16-byte loads per
// lane are 32 registers of data.  As compiled k_sub_write takes 66 VGPRs, i.e. seven wavefronts per SIMD, not eight (forcing
// eight spills two registers; k_sub_count takes 26).  A block of 2,048 events keeps the scan at 24,415 counts for 50 M events.
#pragma once
#include "gx_kept.h"
#include "gx_math.h"

namespace gx {

constexpr int SUB_NT = 256;                          // lanes of a workgroup
constexpr int SUB_NW = SUB_NT / 64;
constexpr int SUB_ITEMS = 8;                         // events in flight per lane
constexpr u32 SUB_BLOCK = SUB_NT * SUB_ITEMS;        // events per block
constexpr u32 SUB_BPC = CNT_CHUNK / SUB_BLOCK;       // blocks per chunk
constexpr u32 SUB_GRID = 2048;                       // most workgroups unless the caller says so: eight per CU
constexpr u32 SUB_MAX_GRID = 65535;                  // ... and the most a caller may force
constexpr int SUB_SCAN_NT = 1024;
static_assert(CNT_CHUNK % SUB_BLOCK == 0, "a chunk is a whole number of blocks");
static_assert(SUB_NW * SUB_ITEMS <= 64, "one wavefront scans a block's (row, wavefront) counts");

struct SubArgs {
  const CntChunk* chunks;
  const u64* first;      // [nChunks] the sample's events before each chunk
  u32 nChunks;
  u64 key;               // subsample_key(seed, sample)
  u64 T;                 // 0 .. 2^32
  u32* blockCnt;         // [nChunks * SUB_BPC]
  const u64* blockOff;   // [nChunks * SUB_BPC + 1]
  uint4* out;
};

__global__ __launch_bounds__(SUB_NT) void k_sub_count(SubArgs a) {
  __shared__ u32 red[SUB_NW];
  const u32 nBlocks = a.nChunks * SUB_BPC;
  for (u32 b = blockIdx.x; b < nBlocks; b += gridDim.x) {
    const u32 c = b / SUB_BPC, b0 = (b % SUB_BPC) * SUB_BLOCK;
    const u32 n = a.chunks[c].n;
    const u64 i0 = a.first[c] + b0;
    u32 kept = 0;
    if (b0 < n) {   // (uniform over the workgroup)
#pragma unroll
      for (int j = 0; j < SUB_ITEMS; j++) {
        const u32 i = b0 + (u32)j * SUB_NT + threadIdx.x;
        kept += i < n && (u64)subsample_draw(a.key, i0 + (u32)j * SUB_NT + threadIdx.x) < a.T;
      }
    }
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      u32 t = 0;
      for (int k = 0; k < SUB_NW; k++) t += red[k];
      a.blockCnt[b] = t;
    }
    __syncthreads();
  }
}

// off[k] = cnt[0] + .. + cnt[k - 1], k = 0 .. n (one workgroup; k_cnt_scan's scheme)
__global__ __launch_bounds__(SUB_SCAN_NT) void k_sub_scan(const u32* __restrict__ cnt, u32 n, u64* __restrict__ off) {
  __shared__ u64 part[SUB_SCAN_NT];
  const u32 per = (n + SUB_SCAN_NT - 1) / SUB_SCAN_NT;
  const u32 lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
  u64 sum = 0;
  for (u32 k = lo; k < hi; k++) sum += cnt[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < SUB_SCAN_NT; o <<= 1) {   // inclusive scan of the threads' sums
    const u64 v = threadIdx.x >= (u32)o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  u64 run = part[threadIdx.x] - sum;
  for (u32 k = lo; k < hi; k++) {
    off[k] = run;
    run += cnt[k];
  }
  if (threadIdx.x == SUB_SCAN_NT - 1) off[n] = part[SUB_SCAN_NT - 1];
}

__global__ __launch_bounds__(SUB_NT) void k_sub_write(SubArgs a) {
  __shared__ u32 cnt[SUB_ITEMS * SUB_NW], pre[SUB_ITEMS * SUB_NW];
  const u32 nBlocks = a.nChunks * SUB_BPC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (u32 b = blockIdx.x; b < nBlocks; b += gridDim.x) {
    const u32 c = b / SUB_BPC, b0 = (b % SUB_BPC) * SUB_BLOCK;
    const CntChunk ch = a.chunks[c];
    if (b0 >= ch.n) continue;   // (uniform over the workgroup: an empty block)
    const u64 i0 = a.first[c] + b0, off = a.blockOff[b];
    uint4 ev[SUB_ITEMS];
    unsigned long long keep[SUB_ITEMS];
#pragma unroll
    for (int j = 0; j < SUB_ITEMS; j++) {
      const u32 i = b0 + (u32)j * SUB_NT + threadIdx.x;
      const bool k = i < ch.n && (u64)subsample_draw(a.key, i0 + (u32)j * SUB_NT + threadIdx.x) < a.T;
      ev[j] = make_uint4(0, 0, 0, 0);
      if (k) ev[j] = kept_event(ch, i);   // (only the kept ones are read: a line is fetched once any of its events is)
      keep[j] = __ballot(k);
      if (lane == 0) cnt[j * SUB_NW + wv] = (u32)__popcll(keep[j]);
    }
    __syncthreads();
    if (wv == 0) {   // exclusive scan of the (row, wavefront) counts, row-major: the kept order
      u32 v = lane < SUB_ITEMS * SUB_NW ? cnt[lane] : 0u;
      const u32 mine = v;
      for (int o = 1; o < SUB_ITEMS * SUB_NW; o <<= 1) {
        const u32 u = __shfl_up(v, o);
        if (lane >= o) v += u;
      }
      if (lane < SUB_ITEMS * SUB_NW) pre[lane] = v - mine;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SUB_ITEMS; j++)
      if ((keep[j] >> lane) & 1ull)
        a.out[off + pre[j * SUB_NW + wv] + (u32)__popcll(keep[j] & ((1ull << lane) - 1))] = ev[j];
    __syncthreads();   // (cnt and pre are the next block's as well)
  }
}

// k_sub_split -- both halves of a sample in one pass (gx_subsample_split_events, gx_subsample_split_kept, gx_reproducibility):
// a stable two-way partition.  Event i goes to half A iff its draw is below T, else to half B; both keep the kept order and
// share one buffer of the sample's n events, A in [0, nA), B in [nA, n).  k_sub_count and k_sub_scan run before it as they do
// before k_sub_write: blockOff[b] is A's offset of block b and blockOff[nBlocks] is nA, read here, so that no count comes
// back to the host between the launches.  B needs no scan of its own: first[c] + b0 events lie before block b of chunk c and
// blockOff[b] of them are A's, so B's part of the block starts at nA + first[c] + b0 - blockOff[b].  Inside a block the valid
// positions pos = j * SUB_NT + threadIdx.x (those below ch.n - b0) are contiguous from 0, so an event with rankA of A's events
// before it has pos - rankA of B's before it; rankA is k_sub_write's (ballot, popcount, the 32-entry scan).  Every event is
// read once and stored once, 16 bytes each way; no workgroup waits for another, every loop is bounded by the chunk list, and
// a place depends on the block offsets alone: the same bytes for every grid.
// As compiled (gfx950, -O3; the compiler's resource-usage remarks) k_sub_split takes 72 VGPRs and no scratch: seven wavefronts
// per SIMD, k_sub_write's step (66 VGPRs, seven as well).  It got there in three moves.  Written as k_sub_write is, with the
// loads made unconditional, it took 76 to 81 and fell to six or five: the chunk's pointer, its count and the block offsets
// came from vector loads (nothing tells the compiler that `out` does not alias them) and sat in vector registers, so they are
// moved to scalar ones (sub_uni); a 64-bit select between the two halves' addresses cost two registers per event, so each
// half has its own store off a uniform base; and the branch on the event form stands once around the eight loads, not inside
// each, so that the packed form's loads are all in flight before the first is unpacked.  Asking for seven by
// __launch_bounds__ instead spilled three registers.
// a value that is the same in every lane, moved to scalar registers (a load the compiler cannot prove uniform lands in vector ones)
__device__ __forceinline__ u32 sub_uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 sub_uni(u64 v) { return ((u64)sub_uni((u32)(v >> 32)) << 32) | sub_uni((u32)v); }

__global__ __launch_bounds__(SUB_NT) void k_sub_split(SubArgs a) {
  __shared__ u32 cnt[SUB_ITEMS * SUB_NW], pre[SUB_ITEMS * SUB_NW];
  const u32 nBlocks = a.nChunks * SUB_BPC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 nA = sub_uni(a.blockOff[nBlocks]);
  for (u32 b = blockIdx.x; b < nBlocks; b += gridDim.x) {
    const u32 c = b / SUB_BPC, b0 = (b % SUB_BPC) * SUB_BLOCK;
    CntChunk ch;
    ch.n = sub_uni(a.chunks[c].n);
    if (b0 >= ch.n) continue;   // (uniform over the workgroup: an empty block)
    ch.p = reinterpret_cast<const void*>(sub_uni((u64)reinterpret_cast<uintptr_t>(a.chunks[c].p)));
    ch.packed = sub_uni(a.chunks[c].packed);
    const u64 i0 = sub_uni(a.first[c]) + b0, offA = sub_uni(a.blockOff[b]), offB = nA + i0 - offA;
    const u32 m = min(ch.n - b0, SUB_BLOCK);   // the block's events: its positions 0 .. m - 1
    uint4 ev[SUB_ITEMS];
    u32 at[SUB_ITEMS];   // A's events before this one in its wavefront's row; bit 31: the event is B's
#pragma unroll
    for (int j = 0; j < SUB_ITEMS; j++) {
      const u32 pos = (u32)j * SUB_NT + threadIdx.x;
      const bool k = pos < m && (u64)subsample_draw(a.key, i0 + pos) < a.T;
      const unsigned long long inA = __ballot(k);
      at[j] = (u32)__popcll(inA & ((1ull << lane) - 1)) | (k ? 0u : 0x80000000u);
      if (lane == 0) cnt[j * SUB_NW + wv] = (u32)__popcll(inA);
    }
    // every event, unconditionally (a position past the end reads the block's last one): one branch on the form around the
    // eight loads, which fly over the scan
    if (ch.packed) {
#pragma unroll
      for (int j = 0; j < SUB_ITEMS; j++) ev[j] = kept_event(ch, b0 + min((u32)j * SUB_NT + threadIdx.x, m - 1));
    } else {
#pragma unroll
      for (int j = 0; j < SUB_ITEMS; j++) ev[j] = kept_event(ch, b0 + min((u32)j * SUB_NT + threadIdx.x, m - 1));
    }
    __syncthreads();
    if (wv == 0) {   // exclusive scan of the (row, wavefront) counts, row-major: the kept order
      u32 v = lane < SUB_ITEMS * SUB_NW ? cnt[lane] : 0u;
      const u32 mine = v;
      for (int o = 1; o < SUB_ITEMS * SUB_NW; o <<= 1) {
        const u32 u = __shfl_up(v, o);
        if (lane >= o) v += u;
      }
      if (lane < SUB_ITEMS * SUB_NW) pre[lane] = v - mine;
    }
    __syncthreads();
    // a store per half: a uniform base and a place below SUB_BLOCK, i.e. one address register per event
    uint4* const outA = a.out + offA;
    uint4* const outB = a.out + offB;
#pragma unroll
    for (int j = 0; j < SUB_ITEMS; j++) {
      const u32 pos = (u32)j * SUB_NT + threadIdx.x;
      const u32 rankA = (pre[j * SUB_NW + wv] + (at[j] & 0x7FFFFFFFu)) & (SUB_BLOCK - 1);
      if (pos < m) {
        if (at[j] & 0x80000000u) outB[(pos - rankA) & (SUB_BLOCK - 1)] = ev[j];
        else outA[rankA] = ev[j];
      }
    }
    __syncthreads();   // (cnt and pre are the next block's as well)
  }
}

}  // namespace gx
