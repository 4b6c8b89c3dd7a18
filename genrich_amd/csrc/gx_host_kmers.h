// gx_host_kmers.h -- the host side of the k-mer count (gx_kmers.h): the refusals, the regions resolved to units (mot_resolve), the
// path by k, the pass in two halves so that several contexts' passes run side by side, the table permuted to the public order and
// checked against the windows; the pass over a caller's regions, over the called peaks and over the genome.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

static_assert(KMER_MAX_K == GX_KMER_MAX_K && KMER_LDS_MAX_K == GX_KMER_LDS_MAX_K, "the header's limits are the kernel's");
static_assert(((size_t)4 << (2 * KMER_LDS_MAX_K)) <= 64 * 1024, "the LDS path's counters fit 64 KiB");

struct KmerGeometry { unsigned grid; u32 step; u64 flushRuns; };

// a pass that is set up: its arguments, its grid, what must live until the stream is drained
struct KmerRun {
  KmerArgs a{};
  unsigned grid = 0;
  bool lds = false;
  size_t nTab = 0;                  // 4^k
  u64 regions = 0;                  // regions that hold at least k bases
  std::vector<MotRegion> rs;
  bool live = false;                // there is something to launch
};

// The public code of a table index ((gc bits) << k | (ag bits), bit j: base x + j): with A = (gc 0, ag 1), C = (1, 0), G = (1, 1),
// T = (0, 0) and the public digits A 0, C 1, G 2, T 3 the digit's high bit is !(gc ^ ag) and its low bit !ag -- linear in the
// bits, so the code is ALL ^ spreadG[gc bits] ^ spreadP[ag bits].  counts[code] = table[index].
void kmer_public(const unsigned long long* table, u32 k, std::vector<uint64_t>& counts) {
  const u32 n = 1u << k, all = (u32)(((u64)1 << (2 * k)) - 1);
  std::vector<u32> sg(n, 0), sp(n, 0);
  for (u32 v = 0; v < n; v++)
    for (u32 j = 0; j < k; j++)
      if ((v >> j) & 1u) {
        sg[v] |= 2u << (2 * (k - 1 - j));
        sp[v] |= 3u << (2 * (k - 1 - j));
      }
  counts.assign((size_t)all + 1, 0);
  for (u32 g = 0; g < n; g++) {
    const unsigned long long* row = table + ((size_t)g << k);
    const u32 cg = all ^ sg[g];
    for (u32 p = 0; p < n; p++) counts[cg ^ sp[p]] = row[p];
  }
}

int kmer_check_k(gx_ctx* ctx, int k) {
  if (k < 1 || k > (int)KMER_MAX_K) return refuse(ctx, "kmers: k must satisfy 1 <= k <= 12");
  return GX_OK;
}

// the refusals, the regions with their units, the grid, the path, the buffers
int kmer_setup(gx_ctx* ctx, const gx_region* reg, size_t n, u32 k, KmerGeometry g, KmerRun& r) {
  ctx->kmLastFlushes = 0;
  if (g.step == 0) g.step = MOT_STEP;
  if (g.flushRuns == 0) g.flushRuns = KMER_FLUSH_RUNS;
  if (g.flushRuns > KMER_FLUSH_RUNS) return refuse(ctx, "kmers: a flush bound must be 1 to 2^25 runs");
  if (n >> 32) return refuse(ctx, "kmers: 2^32 regions or more");
  const char* why = "";
  if (mot_grid(0, g.step, g.grid, &r.grid, &why)) return refuse(ctx, why);   // (the step and the grid, before anything is done)
  if (int rc = gc_current(ctx)) return rc;
  u64 positions = 0;
  const u64 nUnits = mot_resolve(ctx, reg, n, g.step, r.rs, &positions);
  if (mot_grid(nUnits, g.step, g.grid, &r.grid, &why)) return refuse(ctx, why);
  for (const MotRegion& m : r.rs) r.regions += m.end - m.start >= k;
  r.lds = k <= KMER_LDS_MAX_K && !ctx->kmForceHbm;
  r.nTab = (size_t)1 << (2 * k);
  ctx->kmLastPath = r.lds ? 0u : 1u;
  if (r.rs.empty()) return GX_OK;
  hipStream_t s = ctx->stream;
  if (r.lds && !ctx->kmLdsSet) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_kmer_count<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kmer_lds_bytes(KMER_LDS_MAX_K, true)));
    ctx->kmLdsSet = true;
  }
  POOLED(ctx, ctx->kmReg, r.rs.size() * sizeof(MotRegion));
  POOLED(ctx, ctx->kmTable, r.nTab * 8);
  POOLED(ctx, ctx->kmOut, KMC_WORDS * 8);
  HIPCHECK(hipMemcpyAsync(ctx->kmReg.p, r.rs.data(), r.rs.size() * sizeof(MotRegion), hipMemcpyHostToDevice, s));
  KmerArgs& a = r.a;
  a.gc = ctx->gcVec.as<unsigned long long>();
  a.ag = ctx->gcAg.as<unsigned long long>();
  a.acgt = ctx->gcAcgt.as<unsigned long long>();
  a.reg = ctx->kmReg.as<MotRegion>();
  a.nReg = (u32)r.rs.size();
  a.nUnits = (u32)nUnits;
  a.step = g.step;
  a.k = k;
  a.flushRuns = g.flushRuns;
  a.table = ctx->kmTable.as<unsigned long long>();
  a.out = ctx->kmOut.as<unsigned long long>();
  r.live = true;
  return GX_OK;
}

// The pass in two halves: launched with its read-back queued ...
int kmer_begin(gx_ctx* ctx, const gx_region* reg, size_t n, u32 k, KmerGeometry g, KmerRun& r) {
  if (int rc = kmer_setup(ctx, reg, n, k, g, r)) return rc;
  if (!r.live) return GX_OK;
  hipStream_t s = ctx->stream;
  phase_begin(ctx, "kmers");
  HIPCHECK(hipMemsetAsync(ctx->kmTable.p, 0, r.nTab * 8, s));
  HIPCHECK(hipMemsetAsync(ctx->kmOut.p, 0, KMC_WORDS * 8, s));
  const size_t lds = kmer_lds_bytes(k, r.lds);
  if (r.lds) hipLaunchKernelGGL(k_kmer_count<true>, dim3(r.grid), dim3(MOT_NT), lds, s, r.a);
  else hipLaunchKernelGGL(k_kmer_count<false>, dim3(r.grid), dim3(MOT_NT), lds, s, r.a);
  if (int rc__ = dbg_sync(ctx, "k_kmer_count")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  HIPCHECK(ctx->kmHost.ensure((r.nTab + KMC_WORDS) * 8));   // (pinned: the copies are queued, the host goes on to the next context)
  unsigned long long* h = static_cast<unsigned long long*>(ctx->kmHost.p);
  HIPCHECK(hipMemcpyAsync(h, ctx->kmOut.p, KMC_WORDS * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(h + KMC_WORDS, ctx->kmTable.p, r.nTab * 8, hipMemcpyDeviceToHost, s));
  return GX_OK;
}
// ... and drained: the counts in the public order, the windows; their sum is checked
int kmer_end(gx_ctx* ctx, KmerRun& r, std::vector<uint64_t>& counts, u64* windows) {
  *windows = 0;
  if (!r.live) {
    counts.assign(r.nTab, 0);
    return GX_OK;
  }
  HIPCHECK(hipStreamSynchronize(ctx->stream));   // (the regions' host copy may go)
  const unsigned long long* h = static_cast<const unsigned long long*>(ctx->kmHost.p);
  ctx->kmUsed = true;
  ctx->kmLastFlushes = (u32)std::min<unsigned long long>(h[KMC_FLUSHES], 0xffffffffull);
  *windows = h[KMC_WINDOWS];
  kmer_public(h + KMC_WORDS, r.a.k, counts);
  u64 sum = 0;
  for (uint64_t c : counts) sum += c;
  if (sum != *windows) {
    ctx->err = "kmers: the counts do not add up to the windows counted (a lost or doubled contribution)";
    return GX_ERR_ARR;
  }
  return GX_OK;
}

int kmer_pass(gx_ctx* ctx, const gx_region* reg, size_t n, u32 k, KmerGeometry g, std::vector<uint64_t>& counts, u64* windows, u64* regions) {
  KmerRun r;
  if (int rc = kmer_begin(ctx, reg, n, k, g, r)) return rc;
  if (regions) *regions = r.regions;
  return kmer_end(ctx, r, counts, windows);
}

// the peaks gx_find_peaks left on this context, whole (flank < 0) or flank bases to either side of the summit
int kmer_count_peaks(gx_ctx* ctx, u32 k, int flank) {
  const size_t nPk = ctx->nHostPeaks;
  const gx_peak* hp = static_cast<const gx_peak*>(ctx->hPeaks.p);
  std::vector<gx_region> reg(nPk);
  for (size_t i = 0; i < nPk; i++) {
    u64 s = hp[i].start, e = hp[i].end;
    if (flank >= 0) {
      const u64 at = (u64)hp[i].start + hp[i].summit;
      s = std::max<u64>(s, at > (u64)flank ? at - (u64)flank : 0);
      e = std::min<u64>(e, at + (u64)flank + 1);
    }
    reg[i] = gx_region{hp[i].chrom, (u32)s, (u32)e};
  }
  ctx->kmReady = false;
  u64 w = 0, nr = 0;
  if (int rc = kmer_pass(ctx, reg.data(), nPk, k, KmerGeometry{0, 0, 0}, ctx->kmCounts, &w, &nr)) return rc;
  ctx->kmWindows = w;
  ctx->kmRegions = nr;
  ctx->kmK = k;
  ctx->kmReady = true;
  return GX_OK;
}

void drop_kmers(gx_ctx* ctx) {   // gx_reset: the results go, the genome stays
  ctx->kmCounts.clear();
  ctx->kmWindows = ctx->kmRegions = 0;
  ctx->kmReady = ctx->kmUsed = false;
}

}  // namespace
